// b747_eval_body.h -- the body of the evaluation-episode kernels, included once by each of them (b747_eval.h):
// k_eval_episodes (POP = GAINS = false, no `pa`) and k_eval_population.  Textual, not an inlined function: as a
// function the body changed the generated code of k_eval_episodes (profiles/eval_population/isa_diff.txt is taken
// against the library before the population form; the six instantiations stay identical).  In scope where it is
// included: FAST, OD, POP, GAINS, b, cfgc, Cin, ea and, with POP or GAINS, pa.
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
    const float *params = ea.params;
    if constexpr (POP && OD > 0) params += (int64_t)((int)blockIdx.x / pa.waves_per_policy) * pa.policy_stride;
    if constexpr (OD > 0) {
#pragma unroll
        for (int k = 0; k < OD; ++k) o[k] = b.obs[il * OD + k];
        PolicyStage<kOD, kEvalBlock> stage;
        stage.load(params, lane);
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
            const float *pz = params + zoff;
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
            // the lane's own gains, re-read with the command and for its reason (held, they would be eight more
            // doubles live across the policy); every other constant stays the batch's, uniform in SGPRs
            Consts Cl = C;
            if constexpr (GAINS) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (pa.pid_ss) Cl.PID_SS[j] = pa.pid_ss[j * n + il + zy];
                    if (pa.pid_cs) Cl.PID_CS[j] = pa.pid_cs[j * n + il + zy];
                }
            }
            // (the row goes through LDS: a local array became one ten-register value that the allocator
            //  spilled and reloaded whole, 50-60 VGPR spills)
            float *orow = sobs[lane];
            const bool done = env_step_lane<FAST, false, kAllSignals, false, false, double, EvalPush>(
                b, cfg, GAINS ? Cl : C, il, L, a, orow, nullptr, nullptr, r_last, tb, &sg[0][lane], kEvalBlock, st, &push);
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
