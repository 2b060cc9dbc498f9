// b747_eval.h -- whole evaluation episodes in one launch (b747_eval_episodes, include/b747.h).
//
// ControlTestCallback.calc_stepinfo (neural/callbacks.py:60-100) flies one episode per pitch reference with the
// deterministic policy and scores the recorded pitch with calc_stepinfo.  k_eval_episodes does that for 64 envs per
// wave without a history: the policy head (actor_critic<OD, 1>, b747_policy.h) runs in the step loop on the
// observations the last read-out left behind, the generic lane code of b747_lanes.h steps the env (every control
// type / mode, reward, limiter setting and n_sub that k_env_steps covers; run-time constants), and after every DLL
// step the chosen signal goes into the lane's StepInfoAcc (b747_stepinfo.h).  Only B747_NEVAL values per env leave
// the kernel.  Instantiated by two translation units of its own, b747_eval_faithful.hip and b747_eval_fast.hip (the
// FAITHFUL / FAST split of b747_kernels.hip / b747_fast.hip): compiled inside those two, the new kernels changed the
// register allocation and LDS-read scheduling of kernels already there (k_rollout_split<true, ...>).
#pragma once

#include "b747_lanes.h"
#include "b747_policy.h"
#include "b747_stepinfo.h"

#include "b747_eval_args.h"

namespace {

using namespace b747;

// The per-DLL-step hook of env_step_lane: one sample of the scored series per DLL step
struct EvalPush {
    static constexpr bool kEveryStep = true;
    StepInfoAcc &acc;
    int32_t &len;
    int row;
    double scale;
    __device__ __forceinline__ void operator()(const double *sg, int sst) const
    {
        acc.push(scale * nan_to_num(sg[row * sst]), sg[S_SIM_TIME * sst]);
        len += 1;
    }
};

constexpr int kEvalBlock = 64;   // one wave per workgroup: the wave has the SIMD's whole register file
// OD: the policy's obs_dim (3 PID_LIKE, 5 SPEED_MODE), 0 = no policy.  An env's episode ends at its first done or
// after n_env_steps; from then on the lane is frozen (no samples, no return, its state as at the done) while the
// wave's loop runs on for the lanes still live.  Lanes past n step a copy of env n - 1 (the matrix cores need all 64
// lanes) and store nothing.
template <bool FAST, int OD>
__global__ __launch_bounds__(kEvalBlock) B747_NO_FMAC void k_eval_episodes(b747_env_batch b, b747_env_config cfgc,
                                                                           Consts Cin, EvalArgs ea)
{
    constexpr int kOD = OD > 0 ? OD : 1;
    constexpr PolicyDerived PD = PolicyDerived::of(kOD);
    __shared__ __attribute__((aligned(16))) double tb[T_TOTAL];
    __shared__ double sg[NSIG][kEvalBlock];                         // signal stash, [row][lane]
    __shared__ float sobs[kEvalBlock][OBS_MAX_DIM];                 // the read-out's observation rows
    __shared__ float w[OD > 0 ? PD.total : 1];                      // the policy's derived section
    const int lane = threadIdx.x;
    // this variant's table entries, all loads issued at once (as k_model_step with 64-lane workgroups)
    constexpr int lo = FAST ? T_FAST_LO : 0, hi = FAST ? T_TOTAL : T_N;
    constexpr int Q = (hi - lo + kEvalBlock - 1) / kEvalBlock;
    double tv[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int j = lo + lane + q * kEvalBlock;
        tv[q] = (j < hi) ? kTableImage.v[j] : 0.0;
    }
    const EnvCfg &cfg = cfgc;
    const Consts &C = Cin;
    const int64_t n = b.n;
    const int64_t i = (int64_t)blockIdx.x * kEvalBlock + lane;
    const bool owner = i < n;
    const int64_t il = owner ? i : n - 1;
    EnvLane L;
    env_load<double, FAST && kPitchPlane>(b, cfg, il, L, false);
    float o[kOD];
    float a_hold = 0.0f;
    if constexpr (OD > 0) {
#pragma unroll
        for (int k = 0; k < OD; ++k) o[k] = b.obs[il * OD + k];
        PolicyStage<kOD, kEvalBlock> stage;
        stage.load(ea.params, lane);
        stage.store(w, lane);
    } else {
        a_hold = b.action[il];
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int j = lo + lane + q * kEvalBlock;
        if (j < hi) tb[j] = tv[q];
    }
    wg_barrier();
    const bool ctrl0 = (L.s.flags & F_PID_CS) != 0u;
    StepInfoAcc acc;
    acc.init(0.0, ea.error_band);
    int32_t len = 0;
    double itse = 0.0;
    float r_last = 0.0f;
    bool live = true;
    const EvalPush push{acc, len, ea.sig_row, ea.scale};
    for (int32_t st = 0; st < ea.n_env_steps && wave_any(live); ++st) {
        float a = a_hold;
        if constexpr (OD > 0) {   // every lane, live or not: the MFMAs run on the whole wave
            float mean, value;
            // the parameters through an opaque zero, re-derived every step: the loop-invariant fragment and bias
            // loads (~200 VGPRs) would otherwise be hoisted out of the loop and held across the env step.  The
            // matrix-core A fragments come from L2 every step (18 KB per wave), not from an LDS copy: staged in LDS
            // (actor_critic's fr) the kernel took 46 KB per workgroup, three workgroups per CU instead of four, and
            // 65,536 envs (1,024 waves) ran in two rounds -- 29.3 ms against 15.2; at 4 and 4,096 envs 13.8 against 13.7
            int zoff = 0;
#if defined(__HIP_DEVICE_COMPILE__)
            asm volatile("" : "+s"(zoff));
#endif
            const float *pz = ea.params + zoff;
            actor_critic<kOD, 1>(w + zoff, pz, pz + policy_derived_offset(kOD), o, lane, mean, value);
            (void)value;
            a = fminf(fmaxf(mean, ea.act_lo), ea.act_hi);
        }
        if (live) {
            // the command is re-read every env step (through an opaque zero: not hoisted), so that it is not one more
            // value held across the policy and the step (the allocator parked it in an AGPR as a spill)
            int zy = 0;
#if defined(__HIP_DEVICE_COMPILE__)
            asm volatile("" : "+s"(zy));
#endif
            acc.y_base = ea.y_base[il + zy];
            // (the row goes through LDS: a local array became one ten-register value that the allocator
            //  spilled and reloaded whole, 50-60 VGPR spills)
            float *orow = sobs[lane];
            const bool done = env_step_lane<FAST, false, kAllSignals, false, false, double, EvalPush>(
                b, cfg, C, il, L, a, orow, nullptr, nullptr, r_last, tb, &sg[0][lane], kEvalBlock, st, &push);
            itse = sg[S_ITSE][lane];
            if constexpr (OD > 0) {
#pragma unroll
                for (int k = 0; k < OD; ++k) o[k] = orow[k];
            }
            if (done) {
                live = false;
                if (owner) {
                    record_episode_end(b, i, L);
                    // auto_reset is 0 here, so the row of the done step is the terminal observation (EnvReadOut
                    // writes the same values to both); b.obs_dim entries, with a policy or without
                    if (b.terminal_obs) {
                        const int od = OD > 0 ? OD : b.obs_dim;
                        for (int k = 0; k < od; ++k) b.terminal_obs[i * od + k] = orow[k];
                    }
                }
            }
        }
    }
    if (!owner) return;
    env_store<double, FAST && kPitchPlane, false>(b, cfg, i, L, false, ctrl0);
    if constexpr (OD > 0) {
#pragma unroll
        for (int k = 0; k < OD; ++k) b.obs[i * OD + k] = o[k];
    } else {
        // no policy: any observation type.  The lane's LDS row holds its last read-out (every lane is live in its
        // first step, and n_env_steps >= 1 in every launch)
        const int od = b.obs_dim;
        for (int k = 0; k < od; ++k) b.obs[i * od + k] = sobs[lane][k];
    }
    b.reward[i] = r_last;
    b.done[i] = live ? 0 : 1;
    const StepInfo si = acc.finish(ea.y_base[i]);
    ea.out[0 * n + i] = si.overshoot;
    ea.out[1 * n + i] = si.rise_time;
    ea.out[2 * n + i] = si.settling_time;
    ea.out[3 * n + i] = si.static_error;
    ea.out[4 * n + i] = itse;
    ea.out[5 * n + i] = (double)len;
    ea.out[6 * n + i] = L.s.ep_ret;
}

template <bool FAST>
void launch_eval_episodes(const b747_env_batch &b, const b747_env_config &cfg, const Consts &C, const EvalArgs &ea,
                          int od, hipStream_t s)
{
    const dim3 g((unsigned)((b.n + kEvalBlock - 1) / kEvalBlock)), blk(kEvalBlock);
    if (od == 3) hipLaunchKernelGGL((k_eval_episodes<FAST, 3>), g, blk, 0, s, b, cfg, C, ea);
    else if (od == 5) hipLaunchKernelGGL((k_eval_episodes<FAST, 5>), g, blk, 0, s, b, cfg, C, ea);
    else hipLaunchKernelGGL((k_eval_episodes<FAST, 0>), g, blk, 0, s, b, cfg, C, ea);
}

}  // namespace
