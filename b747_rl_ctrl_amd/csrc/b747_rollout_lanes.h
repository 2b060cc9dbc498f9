// b747_rollout_lanes.h -- a whole stochastic PPO rollout in one launch for every env configuration
// (b747_ppo_rollout_lanes, include/b747.h).
//
// b747_ppo_rollout's two-wave kernel (k_rollout_split<true>, b747_ppo_split.h) is specialised on one configuration.
// k_rollout_lanes is the general one: T steps of SB3's collect_rollouts for 64 envs per wave -- the policy
// (actor_critic<OD>), the Gaussian sample of k_policy_act (policy_noise, the same Philox counters), the
// generic lane code of b747_lanes.h for the env step (every control type / mode, reward, limiter setting and n_sub
// that k_env_steps covers; run-time constants), the rollout rows, and k_env_steps' episode end and auto-reset -- with
// the env state and the observation in registers across the steps.  It is k_eval_episodes (b747_eval.h) with noise,
// rows and resets instead of the step-response score, and keeps that kernel's shape: one wave per workgroup, no
// hand-off between waves, one loop bounded by T.  Instantiated by two translation units of its own,
// b747_rollout_lanes_faithful.hip and b747_rollout_lanes_fast.hip (as the evaluation kernel and for its reason: new
// kernels inside an existing unit changed the code generated for the kernels already there).
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/b747.h"
#include "b747_dynamics.h"

namespace b747 {

// Where the value head runs.  obs_dim 3: not in the kernel at all -- the entry point launches k_policy_value<3> over
// the stored rows afterwards (b747_ppo_rollout's deferred pass, which also advances the counter): the batched pass
// costs less than the head does inside the latency-bound step loop (2.14 against 2.31 ms at 4,096 x 64,
// 63.7 against 69.1 ms at 4 x 2,048, within the spread at 65,536 x 64), and gives k_policy_act's bits.  obs_dim 5 has no
// batched value kernel (k_policy_value needs the matrix-core layer 1): in the step loop.
// -DB747_LANES_VALUE_IN_LOOP (diagnostic A/B build only, tools/exp_ppo_rollout_lanes.py --variants): in the loop for both.
#ifdef B747_LANES_VALUE_IN_LOOP
constexpr bool kLanesDeferValue3 = false;
#else
constexpr bool kLanesDeferValue3 = true;
#endif

struct RolloutLanesArgs {
    const float *params;          // packed policy (b747_policy_pack)
    uint64_t seed;
    const uint64_t *step_base;    // nullable = 0; read once per wave, advanced by the launch after this kernel
    int32_t T;
    float act_lo, act_hi;
    float *obs_buf, *act_buf, *logp_buf, *val_buf, *rew_buf;   // row t * n + i ([T][N][obs_dim] for obs_buf)
    uint8_t *done_buf;
};

// Defined in b747_rollout_lanes_fast.hip / b747_rollout_lanes_faithful.hip (hidden: not part of the C ABI); od = the
// policy's obs_dim (3 or 5).  advance (nullable): the counter to add T to, in a one-thread launch after the rollout
// (NULL where the deferred value pass advances it).
__attribute__((visibility("hidden"))) void launch_rollout_lanes_fast(const b747_env_batch &b, const b747_env_config &cfg,
                                                                     const Consts &C, const RolloutLanesArgs &ra, int od,
                                                                     uint64_t *advance, hipStream_t s);
__attribute__((visibility("hidden"))) void launch_rollout_lanes_faithful(const b747_env_batch &b,
                                                                         const b747_env_config &cfg, const Consts &C,
                                                                         const RolloutLanesArgs &ra, int od,
                                                                         uint64_t *advance, hipStream_t s);
}  // namespace b747

#ifndef B747_ROLLOUT_LANES_NO_KERNELS
#include "b747_lanes.h"
#include "b747_policy.h"

namespace {

using namespace b747;

constexpr int kLanesBlock = 64;   // one wave per workgroup: the wave has the SIMD's whole register file

// *step_base += T in a launch of its own, ordered after the rollout kernel: inside that kernel a workgroup that
// starts late would read the advanced base.  (one lane's vector atomic, as k_policy_value's)
template <bool FAST>
__global__ __launch_bounds__(64) void k_step_base_advance(uint64_t *step_base, uint32_t advance)
{
    if (blockIdx.x == 0 && threadIdx.x == 0)
        __hip_atomic_fetch_add(step_base, (uint64_t)advance, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// k_policy_act's sample and its log-probability (b747_policy.h), rounded as written there (that kernel is compiled
// without FMA contraction; so is this, also in the FAST unit: both paths then store the same action bits for the same
// mean and noise)
__device__ __forceinline__ void gaussian_sample(float mean, float log_std, float z, float &a, float &logp)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    a = mean + expf(log_std) * z;
    // log N(a; mean, std) with a - mean = std * z
    logp = -0.5f * z * z - log_std - 0.918938533204672742f;
}

// OD: the policy's obs_dim (3 PID_LIKE, 5 SPEED_MODE).  Lanes past n step a copy of env n - 1 (the matrix cores need
// all 64 lanes) and store nothing: no rollout row, no env buffer, no episode book, no state0 slot.
template <bool FAST, int OD>
__global__ __launch_bounds__(kLanesBlock) B747_NO_FMAC void k_rollout_lanes(b747_env_batch b, b747_env_config cfgc,
                                                                            Consts Cin, RolloutLanesArgs ra)
{
    static_assert(OD == 3 || OD == 5, "k_rollout_lanes: PID_LIKE or SPEED_MODE observations");
    constexpr bool kValueInLoop = !(OD == 3 && kLanesDeferValue3);
    constexpr PolicyDerived PD = PolicyDerived::of(OD);
    __shared__ __attribute__((aligned(16))) double tb[T_TOTAL];
    __shared__ double sg[NSIG][kLanesBlock];                        // signal stash, [row][lane]
    __shared__ float sobs[kLanesBlock][OBS_MAX_DIM];                // the read-out's observation rows
    __shared__ float w[PD.total];                                   // the policy's derived section
    const int lane = threadIdx.x;
    // this variant's table entries, all loads issued at once (as k_eval_episodes)
    constexpr int lo = FAST ? T_FAST_LO : 0, hi = FAST ? T_TOTAL : T_N;
    constexpr int Q = (hi - lo + kLanesBlock - 1) / kLanesBlock;
    double tv[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int j = lo + lane + q * kLanesBlock;
        tv[q] = (j < hi) ? kTableImage.v[j] : 0.0;
    }
    const EnvCfg &cfg = cfgc;
    const Consts &C = Cin;
    const int64_t n = b.n;
    const int64_t i = (int64_t)blockIdx.x * kLanesBlock + lane;
    const bool owner = i < n;
    const int64_t il = owner ? i : n - 1;
    EnvLane L;
    env_load<double, FAST && kPitchPlane>(b, cfg, il, L, false);
    float o[OD];
#pragma unroll
    for (int k = 0; k < OD; ++k) o[k] = b.obs[il * OD + k];
    const uint64_t base = ra.step_base ? *ra.step_base : 0u;
    {
        PolicyStage<OD, kLanesBlock> stage;
        stage.load(ra.params, lane);
        stage.store(w, lane);
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int j = lo + lane + q * kLanesBlock;
        if (j < hi) tb[j] = tv[q];
    }
    wg_barrier();
    const bool ctrl0 = (L.s.flags & F_PID_CS) != 0u;
    const uint64_t env_id = (uint64_t)(b.env_offset + il);
    float a_clip = 0.0f, r_last = 0.0f;
    bool done_last = false, any_reset = false;
    for (int32_t t = 0; t < ra.T; ++t) {
        // every lane, never under a divergent branch: the MFMAs run on the whole wave.  The parameters through an
        // opaque zero, re-derived every step, so that the loop-invariant fragment and bias loads are not hoisted and
        // held across the env step; the A fragments from L2 every step, not from an LDS copy (b747_eval.h has both
        // measurements)
        // Where the value head is in the loop (kValueInLoop), the two heads run one after the other, each a call that
        // keeps one result (the other head's code is dead in it: k_eval_episodes' mean), with a scheduling barrier between them: evaluated together
        // (actor_critic<OD, 3>, as k_policy_act) the scheduler overlaps them, and both heads' fragments, layer-1
        // activations and accumulator tiles on top of the env lane took the kernel past its 512 registers (50-106
        // VGPRs spilled, 204-320 B of scratch, in all four instantiations).  Per head the operations and their order
        // are those of actor_critic<OD, 3>: the same bits.
        float mean, value, other;
        int zoff = 0;
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+s"(zoff));
#endif
        {
            const float *pz = ra.params + zoff;
            actor_critic<OD, 1>(w + zoff, pz, pz + policy_derived_offset(OD), o, lane, mean, other);
        }
#ifdef B747_LANES_SKIP_VALUE
        // Diagnostic build only (with -DB747_LANES_VALUE_IN_LOOP; tools/exp_ppo_rollout_lanes.py --variants; never the
        // product library): no value head at all, val_buf = 0 -- the most a deferred value pass could take out of the loop
        value = 0.0f;
#else
        if constexpr (kValueInLoop) {
#if defined(__HIP_DEVICE_COMPILE__)
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("" : "+s"(zoff));
#endif
            const float *pz = ra.params + zoff;
            actor_critic<OD, 2>(w + zoff, pz, pz + policy_derived_offset(OD), o, lane, other, value);
        } else {
            value = 0.0f;   // (not stored: the deferred pass writes val_buf)
        }
#endif
        (void)other;
        // the sample, its log-probability and the clip: k_policy_act's expressions (b747_policy.h)
        const float z = policy_noise(ra.seed, base + (uint32_t)t, env_id);
        float a, logp;
        gaussian_sample(mean, w[PD.log_std + zoff], z, a, logp);
        a_clip = fminf(fmaxf(a, ra.act_lo), ra.act_hi);
        const int64_t row = (int64_t)t * n + i;
        if (owner) {
#pragma unroll
            for (int k = 0; k < OD; ++k) ra.obs_buf[row * OD + k] = o[k];
            ra.act_buf[row] = a;
            ra.logp_buf[row] = logp;
            if (kValueInLoop) ra.val_buf[row] = value;
        }
        // (the row goes through LDS, not a local array: b747_eval.h)
        float *orow = sobs[lane];
        float *trow = (owner && b.terminal_obs) ? b.terminal_obs + i * OD : nullptr;
        const bool done = env_step_lane<FAST, false, kAllSignals, false, false, double>(
            b, cfg, C, il, L, a_clip, orow, nullptr, trow, r_last, tb, &sg[0][lane], kLanesBlock, t);
#pragma unroll
        for (int k = 0; k < OD; ++k) o[k] = orow[k];
        if (owner) {
            ra.rew_buf[row] = r_last;
            ra.done_buf[row] = done ? 1 : 0;
        }
        done_last = done;
        if (done) {   // as k_env_steps
            if (owner) record_episode_end(b, i, L);
            if (cfg.auto_reset) {
                env_reset_lane(b, cfg, il, L, !any_reset, owner);
                any_reset = true;
            }
        }
    }
    if (!owner) return;
    env_store<double, FAST && kPitchPlane, false>(b, cfg, i, L, any_reset, ctrl0);
#pragma unroll
    for (int k = 0; k < OD; ++k) b.obs[i * OD + k] = o[k];
    b.reward[i] = r_last;
    b.done[i] = done_last ? 1 : 0;
    // (an input of every other call; this one leaves there what b747_policy_act would have: include/b747.h)
    if (b.action) const_cast<float *>(b.action)[i] = a_clip;
}

template <bool FAST>
void launch_rollout_lanes(const b747_env_batch &b, const b747_env_config &cfg, const Consts &C,
                          const RolloutLanesArgs &ra, int od, uint64_t *advance, hipStream_t s)
{
    const dim3 g((unsigned)((b.n + kLanesBlock - 1) / kLanesBlock)), blk(kLanesBlock);
    if (od == 3) hipLaunchKernelGGL((k_rollout_lanes<FAST, 3>), g, blk, 0, s, b, cfg, C, ra);
    else hipLaunchKernelGGL((k_rollout_lanes<FAST, 5>), g, blk, 0, s, b, cfg, C, ra);
    if (advance) hipLaunchKernelGGL((k_step_base_advance<FAST>), dim3(1), dim3(64), 0, s, advance, (uint32_t)ra.T);
}

}  // namespace
#endif  // B747_ROLLOUT_LANES_NO_KERNELS
