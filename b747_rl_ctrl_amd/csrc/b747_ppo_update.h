// b747_ppo_update.h -- one PPO minibatch step on the device: loss, gradient, clip and Adam.
//
// PPO._minibatch (b747_rl_ctrl_amd/ppo.py) for SB3's MlpPolicy as ActorCritic defines it -- separate pi / vf nets
// obs_dim -> 64 -> 64 tanh, action_net, value_net, a state-independent log_std, act_dim 1 -- in four launches:
//   k_ppo_adv_stats   sum and sum of squares of adv[idx] (fp64, shifted by the first element) per block;
//   k_ppo_grad<OD>    per workgroup: the weights in LDS, a loop over 32-row tiles per wave, the gradient of every
//                     parameter and the loss statistics accumulated in registers, one partial vector per workgroup;
//   k_ppo_reduce      the partials summed in a fixed order into grad[P] and stats[8];
//   k_ppo_adam        scale, global L2 norm, clip_grad_norm_'s coefficient and torch.optim.Adam's update on the flat
//                     vector, the step count in a device int64.
// No floating-point atomics: the same inputs give the same bits.  Nothing allocates, synchronises or reads back.
//
// A wave's tile is 32 rows; lane l holds row l & 31, and the half h = l >> 5 holds the 32 units u(ks, h) = (r & 3) +
// 8 (r >> 2) + 32 mt + 4 h (ks = 16 mt + r) -- the rows of the 32x32 MFMA's C/D layout.  The forward (z2 = W2 h1 and
// both tanh) is fp64 on the VALU (upd_forward says why).  The two backward 64x64 products per net (d1 = W2^T delta2,
// dW2 += delta2 h1^T) run on v_mfma_f32_32x32x2_f32: fp32 operands, bit for bit an fp32 fmaf chain.  delta2 is
// computed on the units the lane holds and is the B operand of d1 with no lane movement: the K order of d1 is
// permuted to that unit order (the A fragments in LDS are laid out to match), and its result lands on the units of h1.
// Sums over rows (dW2 on the matrix cores; db2, dW1, db1, the head weights on the VALU) need unit-on-lane operands:
// the wave transposes delta / h through its private LDS scratch (row stride 33: conflict-free reads).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "b747_dynamics.h"
#include "b747_env.h"
#include "b747_policy.h"   // PolicyLayout (flat_params order), PH

namespace b747 {

constexpr int kUpdMaxWG = 256;      // workgroups of k_ppo_grad (one per CU), = partial vectors in the workspace
constexpr int kUpdAdvBlocks = 64;   // blocks of k_ppo_adv_stats
constexpr int kUpdStats = 8;        // pg, vf, entropy loss, clip fraction, approx_kl, |A ratio|, |ratio|+1+|log ratio|, loss
constexpr int kUpdSums = 9;         // fp64 sums over rows: six behind the statistics, then the gradients of
                                    // action_net.bias, value_net.bias and log_std (cancelling sums: fp64 to the end)
constexpr int kUpdTile = 32;        // rows per wave tile (the N of the 32x32 MFMA)
constexpr int kUpdStride = 33;      // row stride of the transposition scratch
constexpr int kUpdAdamBlock = 1024;

// The loss a gradient kernel computes per row (a template / in-scope constant of the shared pieces below; kUpdLossPpo
// compiles to the code they had before there was a second one).  kUpdLossA2c: b747_a2c_update.h -- no ratio, no clip,
// and `idx` may be NULL (the rows 0 .. batch - 1 in order).
constexpr int kUpdLossPpo = 0, kUpdLossA2c = 1;

// Workspace (bytes): [adv partials: double 2 x kUpdAdvBlocks][sum partials: double kUpdSums x kUpdMaxWG]
// [gradient partials: float P x kUpdMaxWG]
B747_HD constexpr int64_t upd_ws_adv() { return 0; }
B747_HD constexpr int64_t upd_ws_sums() { return (int64_t)sizeof(double) * 2 * kUpdAdvBlocks; }
B747_HD constexpr int64_t upd_ws_grad() { return upd_ws_sums() + (int64_t)sizeof(double) * kUpdSums * kUpdMaxWG; }
B747_HD constexpr int64_t upd_ws_bytes(int od)
{
    return upd_ws_grad() + (int64_t)sizeof(float) * PolicyLayout::of(od).total * kUpdMaxWG;
}

// Workgroups of k_ppo_grad / k_pop_grad for a minibatch of `batch` rows (every launcher's grid): two tiles in flight
// per workgroup and net, at most one workgroup per CU
B747_HD constexpr int upd_n_wg(int64_t batch)
{
    const int64_t tiles = (batch + kUpdTile - 1) / kUpdTile, want = (tiles + 1) / 2;
    return (int)(want < kUpdMaxWG ? want : kUpdMaxWG);
}
static_assert(upd_n_wg(2) == 1 && upd_n_wg(64) == 1 && upd_n_wg(65) == 2, "one workgroup per two tiles");
static_assert(upd_n_wg(16320) == 255 && upd_n_wg(16321) == 256 && upd_n_wg(40000) == 256, "at most kUpdMaxWG");
// The member-batched update (b747_ppo_epoch_batched).  One member's slice of its workspace (bytes):
// [adv partials: double 2 x kUpdAdvBlocks][sum partials: double kUpdSums x n_wg][gradient partials: float P x n_wg]
// [the gradient: float P], n_wg = upd_n_wg(batch_size); the slice length is rounded up to 16 bytes
B747_HD constexpr int64_t upd_pop_ws_grad(int64_t batch_size)
{
    return upd_ws_sums() + (int64_t)sizeof(double) * kUpdSums * upd_n_wg(batch_size);
}
B747_HD constexpr int64_t upd_pop_ws_out(int od, int64_t batch_size)
{
    return upd_pop_ws_grad(batch_size) + (int64_t)sizeof(float) * PolicyLayout::of(od).total * upd_n_wg(batch_size);
}
B747_HD constexpr int64_t upd_pop_ws_bytes(int od, int64_t batch_size)
{
    return (upd_pop_ws_out(od, batch_size) + (int64_t)sizeof(float) * PolicyLayout::of(od).total + 15) & ~(int64_t)15;
}
constexpr int kUpdPopMaxMembers = 65535;   // members of one launch: gridDim.y

// Distances between the members of the k_pop_* kernels (member p = blockIdx.y)
struct UpdPopArgs {
    int64_t policy_stride;   // floats: theta
    int64_t n_params;        // floats: m, v
    int64_t n_rows;          // int64: perm
    int64_t ws_stride;       // bytes: the workspace slices
    int64_t stats_stride;    // floats: the statistics rows of one epoch
};

// The obs_dims a policy kernel is instantiated for, written once: with_obs_dim(od, otherwise, f) returns
// f(std::integral_constant<int, od>{}), or `otherwise` for an od not in the list -- every instantiation of f is
// compiled, one is run (as with_bools)
template <int OD>
using obs_dim_c = std::integral_constant<int, OD>;
template <class R, class F>
R with_obs_dim(int od, R otherwise, F &&f)
{
    auto among = [&](auto... c) { return ((od == c() && (otherwise = f(c), true)) || ...); };
    // PID_LIKE, SPEED_MODE, MODEL_STATE, PID_AERO, PID_SPEED_AERO
    among(obs_dim_c<3>{}, obs_dim_c<5>{}, obs_dim_c<7>{}, obs_dim_c<8>{}, obs_dim_c<10>{});
    return otherwise;
}
inline bool policy_obs_dim_ok(int od) { return with_obs_dim(od, false, [](auto) { return true; }); }

// What the launchers take, by name.  The rollout buffers an update reads (rows of T x N, indexed through idx / perm):
struct UpdData {
    const float *obs, *act, *old_logp, *adv, *ret;
};
struct UpdLoss {
    double clip_range, ent_coef, vf_coef;
};
// (the learning rate is not here: a scalar, a host array or a device array, as the entry point has it)
struct UpdAdam {
    double max_grad_norm, beta1, beta2, eps;
};
// One member's optimiser state: the parameters, Adam's moments and step count
struct UpdState {
    float *theta, *m, *v;
    int64_t *t;
};

// Launchers, defined in b747_ppo_update.hip (hidden: not part of the C ABI).  Arguments are validated by the caller;
// an obs_dim without kernels (with_obs_dim) gives hipErrorInvalidValue.
#define B747_HIDDEN __attribute__((visibility("hidden")))
B747_HIDDEN hipError_t launch_ppo_grad(const float *theta, int od, const UpdData &d, const int64_t *idx, int64_t batch,
                                       const UpdLoss &loss, void *workspace, float *grad, float *stats, hipStream_t s);
B747_HIDDEN hipError_t launch_ppo_adam(const UpdState &st, const float *grad, int64_t n_params, double grad_scale,
                                       const UpdAdam &adam, double lr, hipStream_t s);
// Every minibatch of one epoch (b747_ppo_epoch): launch_ppo_grad's launches on perm + j batch_size, then launch_ppo_adam
// with grad_scale 1, for j = 0 .. ceil(n_rows / batch_size) - 1; the first launch error ends the loop and is returned
B747_HIDDEN hipError_t launch_ppo_epoch(const UpdState &st, int od, const UpdData &d, const int64_t *perm, int64_t n_rows,
                                        int64_t batch_size, const UpdLoss &loss, void *workspace, float *grad,
                                        const UpdAdam &adam, double lr, float *stats, hipStream_t s);
// launch_ppo_epoch for member p = 0 .. n_policies - 1 in turn (b747_ppo_epoch_population): its own parameters (st is
// member 0's, theta policy_stride floats apart), moments, step count, sample order, statistics rows and lr[p] (a host
// array); the rollout buffers, the gradient and the workspace are shared (the stream orders the members)
B747_HIDDEN hipError_t launch_ppo_epoch_population(const UpdState &st, int n_policies, int64_t policy_stride, int od,
                                                   const UpdData &d, const int64_t *perm, int64_t n_rows,
                                                   int64_t batch_size, const UpdLoss &loss, void *workspace,
                                                   float *grad, const UpdAdam &adam, const double *lr, float *stats,
                                                   hipStream_t s);
// One epoch of n_policies members, four launches per minibatch for a whole chunk of members (b747_ppo_epoch_batched):
// chunks of min(n_policies, workspace_bytes / upd_pop_ws_bytes, kUpdPopMaxMembers) members, each through all its
// minibatches before the next; lr is a device array; the first launch error ends the loops and is returned
B747_HIDDEN hipError_t launch_ppo_epoch_batched(const UpdState &st, int n_policies, int64_t policy_stride, int od,
                                                const UpdData &d, const int64_t *perm, int64_t n_rows,
                                                int64_t batch_size, const UpdLoss &loss, void *workspace,
                                                int64_t workspace_bytes, const UpdAdam &adam, const double *lr,
                                                float *stats, hipStream_t s);
// The two above with member p's clip_range, ent_coef, vf_coef, max_grad_norm and lr from row p of a hyper-parameter
// table ([n_policies][B747_PPO_HYPER_COLS] doubles, include/b747.h) in place of loss, adam's
// max_grad_norm and lr.  launch_ppo_epoch_population_hyper: a HOST table, each member's scalars to launch_ppo_epoch's
// loop.  launch_ppo_epoch_batched_hyper: a DEVICE table, read by the k_hyp_* kernels by blockIdx.y.
B747_HIDDEN hipError_t launch_ppo_epoch_population_hyper(const UpdState &st, int n_policies, int64_t policy_stride,
                                                         int od, const UpdData &d, const int64_t *perm, int64_t n_rows,
                                                         int64_t batch_size, const double *hyper, void *workspace,
                                                         float *grad, const UpdAdam &adam, float *stats, hipStream_t s);
B747_HIDDEN hipError_t launch_ppo_epoch_batched_hyper(const UpdState &st, int n_policies, int64_t policy_stride, int od,
                                                      const UpdData &d, const int64_t *perm, int64_t n_rows,
                                                      int64_t batch_size, const double *hyper_dev, void *workspace,
                                                      int64_t workspace_bytes, const UpdAdam &adam, float *stats,
                                                      hipStream_t s);
#undef B747_HIDDEN

#ifndef B747_PPO_UPDATE_NO_KERNELS

typedef float upd_f32x16 __attribute__((ext_vector_type(16)));

// The unit held by half h of the wave at index ks of its 32 (the C/D row of register ks & 15 of tile ks >> 4)
B747_HD constexpr int upd_unit(int ks, int h) { return (ks & 3) + 8 * ((ks & 15) >> 2) + 32 * (ks >> 4) + 4 * h; }

// LDS, in floats: the matrix-core A fragments of W2 and W2^T of both nets, the small parameters, per-wave scratch
template <int OD>
struct UpdLds {
    static constexpr int a2 = 0;                       // [net][mt][ks][lane] = W2[32 mt + (lane & 31)][u(ks, lane >> 5)]
    static constexpr int t2 = 2 * 2 * 32 * 64;         // [net][mt][ks][lane] = W2[u(ks, lane >> 5)][32 mt + (lane & 31)]
    static constexpr int sm = 2 * t2;                  // per net: w1[64][OD], b1[64], b2[64], hw[64]; then hb[2], log_std
    static constexpr int net = PH * OD + 3 * PH;
    static constexpr int hb = sm + 2 * net, ls = hb + 2;
    static constexpr int wave = (ls + 1 + 3) & ~3;     // per wave: sa[64][33], sb[64][33], obs[32][OD], g[32]
    static constexpr int sa = 0, sb = PH * kUpdStride, ob = 2 * PH * kUpdStride, g = ob + kUpdTile * OD;
    static constexpr int per_wave = g + kUpdTile;
    static constexpr int total = wave + 4 * per_wave;
    static constexpr int bytes = total * (int)sizeof(float);
    static_assert(PolicyLayout::of(OD).total <= sm, "the cross-wave reduction reuses the fragment region");
    static_assert(bytes <= 160 * 1024, "LDS per CU");
};

// LDS traffic between the lanes of one wave: the wave's LDS operations execute in order, the fences keep the
// compiler from moving them across
__device__ __forceinline__ void upd_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <class T>
__device__ __forceinline__ T upd_half_sum(T x) { return x + __shfl_xor(x, 32); }
template <class T>
__device__ __forceinline__ T upd_wave_sum(T x)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off);
    return x;
}

// The rollout row at position j of the minibatch: idx[j]; for A2C, whose idx may be NULL, j itself then
template <int LOSS>
__device__ __forceinline__ int64_t upd_row(const int64_t *__restrict__ idx, int64_t j)
{
    if constexpr (LOSS == kUpdLossA2c) return idx ? idx[j] : j;
    else return idx[j];
}

// B747_PPO_UPDATE_PIECES_ONLY: the device functions and the kernel bodies' helpers without the PPO kernels themselves,
// for a translation unit that builds kernels of its own from them (b747_a2c_update.hip)
#ifndef B747_PPO_UPDATE_PIECES_ONLY
// Sum and sum of squares of adv[idx[j]] - adv[idx[0]] over the block's share of the minibatch, in fp64
__global__ __launch_bounds__(256) void k_ppo_adv_stats(const float *__restrict__ adv, const int64_t *__restrict__ idx,
                                                       int64_t batch, double *__restrict__ part)
{
    constexpr bool POP = false;
    constexpr int LOSS = kUpdLossPpo;
    constexpr UpdPopArgs pa{0, 0, 0, 0, 0};   // (named by the discarded branch of the body only)
#include "b747_ppo_adv_stats_body.h"
}

// k_ppo_adv_stats for every member of a chunk: grid (kUpdAdvBlocks, members).  idx and part are member 0's.
__global__ __launch_bounds__(256) void k_pop_adv_stats(const float *__restrict__ adv, const int64_t *__restrict__ idx,
                                                       int64_t batch, double *__restrict__ part, UpdPopArgs pa)
{
    constexpr bool POP = true;
    constexpr int LOSS = kUpdLossPpo;
#include "b747_ppo_adv_stats_body.h"
}
#endif  // B747_PPO_UPDATE_PIECES_ONLY

// Accumulators of one net, lane-partial: the dW2 tiles in the C/D layout ([mt][nt]: W2 row 32 mt + C/D row, column
// 32 nt + (lane & 31)); the others for unit 32 mt + (lane & 31), summed over the rows of parity lane >> 5
template <int OD>
struct UpdNetAcc {
    upd_f32x16 w2[2][2];
    float b2[2], w1[2][OD], b1[2], hw[2];
    __device__ __forceinline__ void zero()
    {
#pragma unroll
        for (int a = 0; a < 2; ++a) {
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) w2[a][b][r] = 0.0f;
#pragma unroll
            for (int k = 0; k < OD; ++k) w1[a][k] = 0.0f;
            b2[a] = b1[a] = hw[a] = 0.0f;
        }
    }
};

// tanh in fp64 (exp and one division: ~1e-16 absolute, which is what the forward below needs)
__device__ __forceinline__ double upd_tanh(double x)
{
    const double e = exp(-2.0 * fabs(x));
    return copysign((1.0 - e) / (1.0 + e), x);
}

// Forward of one net for the wave's 32 rows, in fp64 on the VALU: h1 / h2 = the lane's 32 units of its row (rounded
// to fp32 once, for the backward products), out = the head's output (the same in both halves; fp64, unrounded).
// The gradients of the head biases and of log_std are sums over the rows of terms in out that cancel: an fp32
// forward's error in out (~1e-7) shows in them many times enlarged, whichever way it is summed, so the forward --
// 1/3 of the matrix work -- carries fp64 instead.  Layer 2 needs the row's 64 h1: the halves exchange theirs as fp64
// through the wave's scratch ([unit][row], over sa and sb), and its weights are the A fragments of W2, read four output
// units at a time.  h1 (fp32) goes to sb ([unit][row]) for the dW2 product at the end.
template <int OD, int NET>
__device__ __forceinline__ void upd_forward(const float *__restrict__ lds, float *__restrict__ wv, const float (&o)[OD],
                                            int lane, float (&h1)[32], float (&h2)[32], double &out)
{
    using L = UpdLds<OD>;
    const int h = lane >> 5, rl = lane & 31;
    const float *p = lds + L::sm + NET * L::net;
    const float *w1 = p + 4 * h * OD, *b1 = p + PH * OD + 4 * h, *b2 = b1 + PH, *hw = b2 + PH;
    double *d = reinterpret_cast<double *>(wv + L::sa);
    double od[OD];
#pragma unroll
    for (int k = 0; k < OD; ++k) od[k] = (double)o[k];
#pragma unroll
    for (int ks = 0; ks < 32; ++ks) {
        const int u = upd_unit(ks, 0);
        double a = (double)b1[u];
#pragma unroll
        for (int k = 0; k < OD; ++k) a = fma((double)w1[u * OD + k], od[k], a);
        const double t = upd_tanh(a);
        h1[ks] = (float)t;
        d[(u + 4 * h) * kUpdStride + rl] = t;
    }
    upd_wave_sync();
    double z[32];
#pragma unroll
    for (int ks = 0; ks < 32; ++ks) z[ks] = (double)b2[upd_unit(ks, 0)];
    // W2[u(ks, h)][k] = fragment element [mt = ks >> 4][ks' (k)][lane' = (u & 31) + 32 h' (k)], k = u(ks', h')
    const float *a2 = lds + L::a2 + NET * 2 * 32 * 64 + 4 * h;
#pragma unroll 8
    for (int k = 0; k < PH; ++k) {
        const double x = d[k * kUpdStride + rl];
        const float *wk = a2 + (16 * (k >> 5) + (k & 3) + 4 * ((k & 31) >> 3)) * 64 + 32 * ((k >> 2) & 1);
#pragma unroll
        for (int j = 0; j < 8; ++j) {   // output units 16 (j >> 2) + 4 (j & 3) + e: four neighbours in the fragment
            const float4 w = *reinterpret_cast<const float4 *>(wk + (j >> 2) * 32 * 64 + 8 * (j & 3));
            z[4 * j] = fma((double)w.x, x, z[4 * j]);
            z[4 * j + 1] = fma((double)w.y, x, z[4 * j + 1]);
            z[4 * j + 2] = fma((double)w.z, x, z[4 * j + 2]);
            z[4 * j + 3] = fma((double)w.w, x, z[4 * j + 3]);
        }
    }
    double acc = 0.0;
#pragma unroll
    for (int ks = 0; ks < 32; ++ks) {
        const double t = upd_tanh(z[ks]);
        h2[ks] = (float)t;
        acc = fma((double)hw[upd_unit(ks, 0)], t, acc);
    }
    out = upd_half_sum(acc) + (double)lds[L::hb + NET];
    upd_wave_sync();                     // every lane has read the fp64 h1: the scratch is sa and sb again
    float *sbl = wv + L::sb + 4 * h * kUpdStride + rl;
#pragma unroll
    for (int ks = 0; ks < 32; ++ks) sbl[upd_unit(ks, 0) * kUpdStride] = h1[ks];
}

// Backward of one net from g = dLoss/d out per row (0 for a row past the minibatch), into the accumulators
template <int OD, int NET>
__device__ __forceinline__ void upd_backward(const float *__restrict__ lds, float *__restrict__ wv, int lane, float g,
                                             const float (&h1)[32], float (&h2)[32], UpdNetAcc<OD> &acc)
{
    using L = UpdLds<OD>;
    const int h = lane >> 5, rl = lane & 31;
    const float *hw = lds + L::sm + NET * L::net + PH * OD + 2 * PH + 4 * h;
    float *sa = wv + L::sa, *sb = wv + L::sb, *ob = wv + L::ob, *gs = wv + L::g;
    float *sal = sa + 4 * h * kUpdStride + rl;            // write: [u(ks, h)][row]
    const float *sar = sa + rl * kUpdStride + h;          // read:  [unit rl (+ 32)][row 2 s + h]
    const float *sbr = sb + rl * kUpdStride + h;
    // head weights: sum over rows of g h2
#pragma unroll
    for (int ks = 0; ks < 32; ++ks) sal[upd_unit(ks, 0) * kUpdStride] = h2[ks];
    if (h == 0) gs[rl] = g;
    upd_wave_sync();
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        const float gg = gs[2 * s + h];
        acc.hw[0] = fmaf(gg, sar[2 * s], acc.hw[0]);
        acc.hw[1] = fmaf(gg, sar[32 * kUpdStride + 2 * s], acc.hw[1]);
    }
    upd_wave_sync();
    // delta2 = g hw (1 - h2^2), in place of h2; d1 = W2^T delta2
#pragma unroll
    for (int ks = 0; ks < 32; ++ks) {
        h2[ks] = (g * hw[upd_unit(ks, 0)]) * fmaf(-h2[ks], h2[ks], 1.0f);
        sal[upd_unit(ks, 0) * kUpdStride] = h2[ks];
    }
    upd_f32x16 d1[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) d1[0][r] = d1[1][r] = 0.0f;
    const float *t2 = lds + L::t2 + NET * 2 * 32 * 64 + lane;
#pragma unroll
    for (int ks = 0; ks < 32; ++ks) {
        d1[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(t2[ks * 64], h2[ks], d1[0], 0, 0, 0);
        d1[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(t2[(32 + ks) * 64], h2[ks], d1[1], 0, 0, 0);
    }
    upd_wave_sync();
    // dW2 += delta2 h1^T (K = the tile's rows), db2 += the A operands
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        const float a0 = sar[2 * s], a1 = sar[32 * kUpdStride + 2 * s];
        const float b0 = sbr[2 * s], b1 = sbr[32 * kUpdStride + 2 * s];
        acc.w2[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc.w2[0][0], 0, 0, 0);
        acc.w2[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc.w2[0][1], 0, 0, 0);
        acc.w2[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc.w2[1][0], 0, 0, 0);
        acc.w2[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc.w2[1][1], 0, 0, 0);
        acc.b2[0] += a0;
        acc.b2[1] += a1;
    }
    upd_wave_sync();
    // delta1 = d1 (1 - h1^2); dW1 += delta1 obs^T, db1 += delta1
#pragma unroll
    for (int ks = 0; ks < 32; ++ks)
        sal[upd_unit(ks, 0) * kUpdStride] = d1[ks >> 4][ks & 15] * fmaf(-h1[ks], h1[ks], 1.0f);
    upd_wave_sync();
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        const float e0 = sar[2 * s], e1 = sar[32 * kUpdStride + 2 * s];
        acc.b1[0] += e0;
        acc.b1[1] += e1;
#pragma unroll
        for (int k = 0; k < OD; ++k) {
            const float x = ob[(2 * s + h) * OD + k];
            acc.w1[0][k] = fmaf(e0, x, acc.w1[0][k]);
            acc.w1[1][k] = fmaf(e1, x, acc.w1[1][k]);
        }
    }
    upd_wave_sync();
}

// A wave's accumulators of one net into the workgroup's gradient vector in LDS (flat_params order): first = store,
// otherwise add (the waves take turns, in wave order)
template <int OD, int NET>
__device__ __forceinline__ void upd_flush(float *__restrict__ out, int lane, const UpdNetAcc<OD> &acc, bool first)
{
    constexpr PolicyLayout P = PolicyLayout::of(OD);
    constexpr int w1 = NET ? P.vf_w1 : P.pi_w1, b1 = NET ? P.vf_b1 : P.pi_b1, w2 = NET ? P.vf_w2 : P.pi_w2;
    constexpr int b2 = NET ? P.vf_b2 : P.pi_b2, hw = NET ? P.wv : P.wa, hb = NET ? P.bv : P.ba;
    const int h = lane >> 5, rl = lane & 31;
    auto put = [&](int i, float v) { out[i] = first ? v : out[i] + v; };
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) put(w2 + (upd_unit(16 * mt + r, 0) + 4 * h) * PH + 32 * nt + rl, acc.w2[mt][nt][r]);
        const float vb2 = upd_half_sum(acc.b2[mt]), vb1 = upd_half_sum(acc.b1[mt]), vhw = upd_half_sum(acc.hw[mt]);
        float vw1[OD];
#pragma unroll
        for (int k = 0; k < OD; ++k) vw1[k] = upd_half_sum(acc.w1[mt][k]);
        if (h == 0) {
            const int u = 32 * mt + rl;
            put(b2 + u, vb2);
            put(b1 + u, vb1);
            put(hw + u, vhw);
#pragma unroll
            for (int k = 0; k < OD; ++k) put(w1 + u * OD + k, vw1[k]);
        }
    }
    if (lane == 0 && first) out[hb] = 0.0f;   // (the head's bias gradient travels with the fp64 sums)
}

struct UpdRowArgs {
    const float *obs, *act, *old_logp, *adv, *ret;
    const int64_t *idx;
    int64_t batch;
    double clip, vf_coef, adv_mean, adv_inv;
};

// One net (0 policy, 1 value) over the tiles first, first + stride, ...: forward, the row's loss terms, backward.
// LOSS selects the policy net's row math (the value net's is the same for both): kUpdLossPpo the clipped surrogate;
// kUpdLossA2c -A logp with g_logp = -A / B on every row, the sums A logp in slot 0 and |A logp| in slot 4, slots 2, 3
// and 5 left 0, old_logp and clip not read.
template <int OD, int NET, int LOSS = kUpdLossPpo>
__device__ __forceinline__ void upd_tiles(const float *__restrict__ lds, float *__restrict__ wv, const UpdRowArgs &a,
                                          int lane, int64_t first, int64_t stride, UpdNetAcc<OD> &acc,
                                          double (&sums)[kUpdSums])
{
    using L = UpdLds<OD>;
    const int h = lane >> 5, rl = lane & 31;
    const float log_std = lds[L::ls];
    const double inv_var = exp(-2.0 * (double)log_std), inv_b = 1.0 / (double)a.batch;
    const int64_t tiles = (a.batch + kUpdTile - 1) / kUpdTile;
#pragma unroll 1
    for (int64_t tile = first; tile < tiles; tile += stride) {
        const int64_t j = tile * kUpdTile + rl;
        const bool valid = j < a.batch, count = valid && h == 0;
        const int64_t row = upd_row<LOSS>(a.idx, valid ? j : a.batch - 1);
        float o[OD];
#pragma unroll
        for (int k = 0; k < OD; ++k) o[k] = a.obs[row * OD + k];
        if (h == 0) {
#pragma unroll
            for (int k = 0; k < OD; ++k) wv[L::ob + rl * OD + k] = o[k];
        }
        // the row's loss terms from the fp32 forward in fp64 (one row per lane: nothing beside the nets' work), so
        // that the sums that cancel -- the head biases' and log_std's gradients -- carry the forward's error only
        float h1[32], h2[32];
        double out, g;
        if constexpr (NET == 0 && LOSS == kUpdLossA2c) {
            const double a_row = (double)a.act[row];
            const double an = ((double)a.adv[row] - a.adv_mean) * a.adv_inv;   // (mean 0, factor 1: adv itself, exactly)
            upd_forward<OD, 0>(lds, wv, o, lane, h1, h2, out);
            const double diff = a_row - out, q = diff * diff * inv_var;
            const double logp = (-0.5 * q - (double)log_std) - 0.918938533204672742;
            const double g_logp = valid ? -(an * inv_b) : 0.0;
            if (count) {
                sums[0] += an * logp;
                sums[4] += fabs(an * logp);
                sums[8] += g_logp * (q - 1.0);
            }
            g = g_logp * (diff * inv_var);
        } else if constexpr (NET == 0) {
            const double a_row = (double)a.act[row], olp = (double)a.old_logp[row];
            const double an = ((double)a.adv[row] - a.adv_mean) * a.adv_inv;
            upd_forward<OD, 0>(lds, wv, o, lane, h1, h2, out);
            const double diff = a_row - out, q = diff * diff * inv_var;
            const double logp = (-0.5 * q - (double)log_std) - 0.918938533204672742;
            const double lr = logp - olp, ratio = exp(lr);
            const double rc = ratio < 1.0 - a.clip ? 1.0 - a.clip : (ratio > 1.0 + a.clip ? 1.0 + a.clip : ratio);
            const double s1 = an * ratio, s2 = an * rc;
            const double g_logp = (valid && s1 <= s2) ? -(s1 * inv_b) : 0.0;
            if (count) {
                sums[0] += s1 < s2 ? s1 : s2;
                sums[2] += fabs(ratio - 1.0) > a.clip ? 1.0 : 0.0;
                sums[3] += (ratio - 1.0) - lr;
                sums[4] += fabs(s1);
                sums[5] += (fabs(ratio) + 1.0) + fabs(lr);
                sums[8] += g_logp * (q - 1.0);
            }
            g = g_logp * (diff * inv_var);
        } else {
            const double rt = (double)a.ret[row];
            upd_forward<OD, 1>(lds, wv, o, lane, h1, h2, out);
            const double err = rt - out;
            if (count) sums[1] += err * err;
            g = valid ? (-2.0 * a.vf_coef * inv_b) * err : 0.0;
        }
        if (h == 0) sums[6 + NET] += g;
        upd_backward<OD, NET>(lds, wv, lane, (float)g, h1, h2, acc);
    }
}

#ifndef B747_PPO_UPDATE_PIECES_ONLY
// See the head of the file.  sums (per workgroup, fp64): min(A ratio, A clamp(ratio)), (ret - value)^2, [|ratio - 1|
// > clip], (ratio - 1) - log ratio, |A ratio|, |ratio| + 1 + |log ratio| over the workgroup's rows, then dLoss/d mean,
// dLoss/d value and dLoss/d log_std summed over them.
template <int OD>
__global__ __launch_bounds__(256) void k_ppo_grad(const float *__restrict__ theta, const float *__restrict__ obs,
                                                  const float *__restrict__ act, const float *__restrict__ old_logp,
                                                  const float *__restrict__ adv, const float *__restrict__ ret,
                                                  const int64_t *__restrict__ idx, int64_t batch, double clip,
                                                  double vf_coef,
                                                  const double *__restrict__ adv_part, float *__restrict__ gpart,
                                                  double *__restrict__ spart)
{
    constexpr bool POP = false;
    constexpr int LOSS = kUpdLossPpo;
    constexpr UpdPopArgs pa{0, 0, 0, 0, 0};   // (named by the discarded branch of the body only)
#include "b747_ppo_grad_body.h"
}

// k_ppo_grad<OD> for every member of a chunk: grid (n_wg, members), n_wg what the member's own launch has.  theta,
// idx and the three workspace pointers are member 0's.
template <int OD>
__global__ __launch_bounds__(256) void k_pop_grad(const float *__restrict__ theta, const float *__restrict__ obs,
                                                  const float *__restrict__ act, const float *__restrict__ old_logp,
                                                  const float *__restrict__ adv, const float *__restrict__ ret,
                                                  const int64_t *__restrict__ idx, int64_t batch, double clip,
                                                  double vf_coef,
                                                  const double *__restrict__ adv_part, float *__restrict__ gpart,
                                                  double *__restrict__ spart, UpdPopArgs pa)
{
    constexpr bool POP = true;
    constexpr int LOSS = kUpdLossPpo;
#include "b747_ppo_grad_body.h"
}

// grad[i] = the partials' sum in workgroup order (fp64, rounded once); the last thread turns the row sums into
// PPO._minibatch's statistics and the loss.  The entropy term's gradient (-ent_coef on log_std) joins here.
__global__ __launch_bounds__(256) void k_ppo_reduce(const float *__restrict__ gpart, const double *__restrict__ spart,
                                                    int n_wg, int n_params, int ba_at, int bv_at, int log_std_at,
                                                    const float *__restrict__ theta, int64_t batch, float ent_coef,
                                                    float vf_coef, float *__restrict__ grad, float *__restrict__ stats)
{
    constexpr bool POP = false;
    constexpr UpdPopArgs pa{0, 0, 0, 0, 0};   // (named by the discarded branch of the body only)
#include "b747_ppo_reduce_body.h"
}

// k_ppo_reduce for every member of a chunk: grid (ceil((n_params + 1) / 256), members).  gpart, spart, grad (in the
// workspace), theta and stats are member 0's.
__global__ __launch_bounds__(256) void k_pop_reduce(const float *__restrict__ gpart, const double *__restrict__ spart,
                                                    int n_wg, int n_params, int ba_at, int bv_at, int log_std_at,
                                                    const float *__restrict__ theta, int64_t batch, float ent_coef,
                                                    float vf_coef, float *__restrict__ grad, float *__restrict__ stats,
                                                    UpdPopArgs pa)
{
    constexpr bool POP = true;
#include "b747_ppo_reduce_body.h"
}

// clip_grad_norm_ + torch.optim.Adam (no weight decay, no amsgrad) on the flat vector: g = grad_scale grad,
// coef = min(1, max_norm / (|g| + 1e-6)), t += 1, m = m + (1 - b1)(g - m), v = b2 v + (1 - b2) g^2,
// theta -= (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps).  Element arithmetic in fp64, stored as fp32.
__global__ __launch_bounds__(kUpdAdamBlock) void k_ppo_adam(float *__restrict__ theta, float *__restrict__ m,
                                                            float *__restrict__ v, int64_t *__restrict__ t,
                                                            const float *__restrict__ grad, int64_t n, double grad_scale,
                                                            double max_norm, double lr, double beta1, double beta2,
                                                            double eps)
{
    constexpr bool POP = false;
    constexpr UpdPopArgs pa{0, 0, 0, 0, 0};   // (named by the discarded branch of the body only)
#include "b747_ppo_adam_body.h"
}

// k_ppo_adam for every member of a chunk: grid (1, members), one workgroup per member.  theta, m, v, t, grad (in the
// workspace) and lr_dev are member 0's; the member's learning rate comes from the device array.
__global__ __launch_bounds__(kUpdAdamBlock) void k_pop_adam(float *__restrict__ theta, float *__restrict__ m,
                                                            float *__restrict__ v, int64_t *__restrict__ t,
                                                            const float *__restrict__ grad, int64_t n, double grad_scale,
                                                            double max_norm, const double *__restrict__ lr_dev,
                                                            double beta1, double beta2, double eps, UpdPopArgs pa)
{
    constexpr bool POP = true;
    const double lr = lr_dev[blockIdx.y];
#include "b747_ppo_adam_body.h"
}

// ---- the member-batched kernels with per-member hyper-parameters (b747_ppo_epoch_batched_hyper).
// As k_pop_adam does for lr: member p = blockIdx.y loads its values from row p of the device table (hyper_dev is
// member 0's row; B747_PPO_HYPER_* name the columns) into locals named as the body expects, then runs the unchanged
// text with POP.  The loads are workgroup-uniform: scalar loads, SGPRs.  k_pop_adv_stats reads no hyper-parameter.

// k_pop_grad<OD> with the member's clip and vf_coef from the table
template <int OD>
__global__ __launch_bounds__(256) void k_hyp_grad(const float *__restrict__ theta, const float *__restrict__ obs,
                                                  const float *__restrict__ act, const float *__restrict__ old_logp,
                                                  const float *__restrict__ adv, const float *__restrict__ ret,
                                                  const int64_t *__restrict__ idx, int64_t batch,
                                                  const double *__restrict__ hyper_dev,
                                                  const double *__restrict__ adv_part, float *__restrict__ gpart,
                                                  double *__restrict__ spart, UpdPopArgs pa)
{
    constexpr bool POP = true;
    const double *hyp = hyper_dev + (int64_t)blockIdx.y * B747_PPO_HYPER_COLS;
    const double clip = hyp[B747_PPO_HYPER_CLIP_RANGE], vf_coef = hyp[B747_PPO_HYPER_VF_COEF];
    constexpr int LOSS = kUpdLossPpo;
#include "b747_ppo_grad_body.h"
}

// k_pop_reduce with the member's ent_coef and vf_coef from the table, rounded to float here (the launcher's rounding
// of k_pop_reduce's arguments)
__global__ __launch_bounds__(256) void k_hyp_reduce(const float *__restrict__ gpart, const double *__restrict__ spart,
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

// k_pop_adam with the member's max_norm and lr from the table
__global__ __launch_bounds__(kUpdAdamBlock) void k_hyp_adam(float *__restrict__ theta, float *__restrict__ m,
                                                            float *__restrict__ v, int64_t *__restrict__ t,
                                                            const float *__restrict__ grad, int64_t n, double grad_scale,
                                                            const double *__restrict__ hyper_dev, double beta1,
                                                            double beta2, double eps, UpdPopArgs pa)
{
    constexpr bool POP = true;
    const double *hyp = hyper_dev + (int64_t)blockIdx.y * B747_PPO_HYPER_COLS;
    const double max_norm = hyp[B747_PPO_HYPER_MAX_GRAD_NORM], lr = hyp[B747_PPO_HYPER_LR];
#include "b747_ppo_adam_body.h"
}

#endif  // B747_PPO_UPDATE_PIECES_ONLY

#endif  // B747_PPO_UPDATE_NO_KERNELS

}  // namespace b747
