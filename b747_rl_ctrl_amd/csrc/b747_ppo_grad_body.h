// b747_ppo_grad_body.h -- the body of k_ppo_grad<OD> and of its member-batched sibling k_pop_grad<OD>
// (b747_ppo_update.h).  Textual, not an inlined function, as b747_eval_body.h: the existing kernels keep their
// instruction streams.  In scope where it is included: OD, POP, LOSS (kUpdLossPpo, or kUpdLossA2c for k_a2c_grad<OD>,
// b747_a2c_update.hip, and k_apop_grad<OD>, b747_a2c_population.hip), the arguments of k_ppo_grad and pa (read with POP
// only).
// POP: member p = blockIdx.y reads its own parameters and perm row and writes its own slice of the workspace --
// workgroup-uniform offsets, applied once here; blockIdx.x and gridDim.x are what a launch of the member alone has.
    if constexpr (POP) {
        const int64_t ws_off = (int64_t)blockIdx.y * pa.ws_stride;
        theta += (int64_t)blockIdx.y * pa.policy_stride;
        idx += (int64_t)blockIdx.y * pa.n_rows;
        if (LOSS != kUpdLossA2c || adv_part)   // (A2C's NULL -- no normalize_advantage -- stays NULL for every member)
            adv_part = reinterpret_cast<const double *>(reinterpret_cast<const char *>(adv_part) + ws_off);
        gpart = reinterpret_cast<float *>(reinterpret_cast<char *>(gpart) + ws_off);
        spart = reinterpret_cast<double *>(reinterpret_cast<char *>(spart) + ws_off);
    }
    using L = UpdLds<OD>;
    constexpr PolicyLayout P = PolicyLayout::of(OD);
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ double adv_ms[2];          // mean, 1 / (std + 1e-8)
    __shared__ double wsum[4][kUpdSums];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // ---- stage the parameters
    for (int e = tid; e < 2 * 2 * 32 * 64; e += 256) {
        const int net = e >> 12, mt = (e >> 11) & 1, ks = (e >> 6) & 31, l = e & 63;
        const int w2 = net ? P.vf_w2 : P.pi_w2, u = upd_unit(ks, l >> 5), i = 32 * mt + (l & 31);
        lds[L::a2 + e] = theta[w2 + i * PH + u];
        lds[L::t2 + e] = theta[w2 + u * PH + i];
    }
    for (int e = tid; e < PH * OD; e += 256) {
        lds[L::sm + e] = theta[P.pi_w1 + e];
        lds[L::sm + L::net + e] = theta[P.vf_w1 + e];
    }
    if (tid < PH) {
        float *p0 = lds + L::sm + PH * OD, *p1 = p0 + L::net;
        p0[tid] = theta[P.pi_b1 + tid];
        p0[PH + tid] = theta[P.pi_b2 + tid];
        p0[2 * PH + tid] = theta[P.wa + tid];
        p1[tid] = theta[P.vf_b1 + tid];
        p1[PH + tid] = theta[P.vf_b2 + tid];
        p1[2 * PH + tid] = theta[P.wv + tid];
    }
    if (tid == 64) {
        lds[L::hb] = theta[P.ba];
        lds[L::hb + 1] = theta[P.bv];
        lds[L::ls] = theta[P.log_std];
    }
    // the minibatch's advantage statistics from the blocks' partial sums, in block order (A2C with adv_part NULL -- no
    // normalize_advantage, no statistics launch: mean 0 and factor 1, A = adv)
    if (tid == 0 && LOSS == kUpdLossA2c && !adv_part) {
        adv_ms[0] = 0.0;
        adv_ms[1] = 1.0;
    } else if (tid == 0) {
        double s = 0.0, q = 0.0;
        for (int b = 0; b < kUpdAdvBlocks; ++b) {
            s += adv_part[2 * b];
            q += adv_part[2 * b + 1];
        }
        const double n = (double)batch, var = (q - s * s / n) / (n - 1.0);
        adv_ms[0] = (double)adv[upd_row<LOSS>(idx, 0)] + s / n;
        adv_ms[1] = 1.0 / (sqrt(var > 0.0 ? var : 0.0) + 1e-8);
    }
    __syncthreads();

    // waves 0 / 1 take the policy net, waves 2 / 3 the value net (one net's accumulators per wave); each pair of
    // waves walks every tile of the workgroup's share
    float *wv = lds + L::wave + wave * L::per_wave;
    UpdNetAcc<OD> acc;
    acc.zero();
    double sums[kUpdSums] = {};
    const UpdRowArgs ra{obs, act, old_logp, adv, ret, idx, batch, clip, vf_coef, adv_ms[0], adv_ms[1]};
    if (wave < 2) upd_tiles<OD, 0, LOSS>(lds, wv, ra, lane, blockIdx.x * 2 + (wave & 1), gridDim.x * 2, acc, sums);
    else upd_tiles<OD, 1, LOSS>(lds, wv, ra, lane, blockIdx.x * 2 + (wave & 1), gridDim.x * 2, acc, sums);

    // ---- the waves' accumulators into one vector (waves 0 and 2 store their net's part, then 1 and 3 add theirs)
    __syncthreads();                     // every wave is done with the fragments: their region becomes the vector
#pragma unroll 1
    for (int w = 0; w < 2; ++w) {
        if ((wave & 1) == w) {
            if (wave < 2) {
                upd_flush<OD, 0>(lds, lane, acc, w == 0);
                if (lane == 0 && w == 0) lds[P.log_std] = 0.0f;
            } else {
                upd_flush<OD, 1>(lds, lane, acc, w == 0);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < kUpdSums; ++k) {
        const double v = upd_wave_sum(sums[k]);
        if (lane == 0) wsum[wave][k] = v;
    }
    __syncthreads();
    for (int e = tid; e < P.total; e += 256) gpart[(int64_t)blockIdx.x * P.total + e] = lds[e];
    if (tid < kUpdSums)
        spart[blockIdx.x * kUpdSums + tid] = ((wsum[0][tid] + wsum[1][tid]) + wsum[2][tid]) + wsum[3][tid];
