// b747_rollout_lanes_body.h -- the body of the one-wave PPO rollout kernels, included once by each of them:
// k_rollout_lanes (b747_rollout_lanes.h: POP = REW = false, no `pa`) and k_rollout_population
// (b747_rollout_population.h).  Textual, not an inlined function, as b747_eval_body.h and for its reason: the four
// k_rollout_lanes instantiations keep their instruction streams (profiles/ppo_rollout_population/isa_diff.txt is
// taken against the library before the population form).  In scope where it is included: FAST, OD, POP, REW, b,
// cfgc, Cin, ra and, with POP or REW, pa.
    static_assert(OD == 3 || OD == 5, "the one-wave rollout kernels: PID_LIKE or SPEED_MODE observations");
    // (the population form: always in the loop -- k_policy_value<3>'s deferred pass takes one policy for all rows)
    constexpr bool kValueInLoop = POP || !(OD == 3 && kLanesDeferValue3);
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
    // POP: the wave's own policy and reward row -- wave-uniform addresses, computed once here
    const float *params = ra.params;
    if constexpr (POP) params += (int64_t)((int)blockIdx.x / pa.waves_per_policy) * pa.policy_stride;
    // REW: the wave flies with a private configuration whose reward constants are its group's row.  Loaded here,
    // before the kernel's first store, so that the loads are scalar (a wave-uniform address that nothing has
    // written: s_load) and the eight doubles stay in SGPRs across the steps -- the registers of the kernel without
    // REW.  (Re-read every env step through an opaque zero, as b747_eval_body.h's gains, they became four
    // global_load_dwordx4 per step: after the loop's stores the compiler no longer takes the row for unwritten; 6
    // AGPRs more in FAST obs_dim 5, 16 in FAITHFUL.)  Only the reward reads rew (b747_env.h); the resets do not.
    EnvCfg cfgl = cfgc;
    if constexpr (REW) {
        const double *rew_row = pa.rew_pop + (int64_t)((int)blockIdx.x / pa.waves_per_policy) * 8;
#pragma unroll
        for (int j = 0; j < 8; ++j) cfgl.rew[j] = rew_row[j];
    }
    {
        PolicyStage<OD, kLanesBlock> stage;
        stage.load(params, lane);
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
            const float *pz = params + zoff;
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
            const float *pz = params + zoff;
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
            b, REW ? cfgl : cfg, C, il, L, a_clip, orow, nullptr, trow, r_last, tb, &sg[0][lane], kLanesBlock, t);
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
    if constexpr (POP) {
        // the bootstrap value of the observation the rollout ends on: the value head once more, every lane (the
        // MFMAs run on the whole wave) -- actor_critic<OD, 2>'s operations, so b747_policy_act's value_out on b.obs
        if (pa.last_val) {   // (uniform)
            float other, value;
            int zoff = 0;
#if defined(__HIP_DEVICE_COMPILE__)
            asm volatile("" : "+s"(zoff));
#endif
            const float *pz = params + zoff;
            actor_critic<OD, 2>(w + zoff, pz, pz + policy_derived_offset(OD), o, lane, other, value);
            (void)other;
            if (owner) pa.last_val[i] = value;
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
