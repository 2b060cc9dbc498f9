// b747_ppo_reduce_body.h -- the body of k_ppo_reduce and of its member-batched sibling k_pop_reduce
// (b747_ppo_update.h).  Textual, not an inlined function, as b747_eval_body.h: the existing kernel keeps its
// instruction stream.  In scope where it is included: POP, the arguments of k_ppo_reduce and pa (read with POP only).
// POP: member p = blockIdx.y sums its own partials into the gradient vector of its workspace slice and writes its own
// statistics row.
    if constexpr (POP) {
        const int64_t ws_off = (int64_t)blockIdx.y * pa.ws_stride;
        gpart = reinterpret_cast<const float *>(reinterpret_cast<const char *>(gpart) + ws_off);
        spart = reinterpret_cast<const double *>(reinterpret_cast<const char *>(spart) + ws_off);
        grad = reinterpret_cast<float *>(reinterpret_cast<char *>(grad) + ws_off);
        theta += (int64_t)blockIdx.y * pa.policy_stride;
        stats += (int64_t)blockIdx.y * pa.stats_stride;
    }
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n_params) {
        double a = 0.0;
        const int k = i == ba_at ? 6 : (i == bv_at ? 7 : (i == log_std_at ? 8 : -1));   // the three fp64 sums
        if (k >= 0) {
            for (int w = 0; w < n_wg; ++w) a += spart[w * kUpdSums + k];
        } else {
#pragma unroll 8
            for (int w = 0; w < n_wg; ++w) a += (double)gpart[(int64_t)w * n_params + i];
        }
        if (i == log_std_at) a -= (double)ent_coef;
        grad[i] = (float)a;
    } else if (i == n_params) {
        double s[kUpdSums] = {};
        for (int w = 0; w < n_wg; ++w)
#pragma unroll
            for (int k = 0; k < kUpdSums; ++k) s[k] += spart[w * kUpdSums + k];
        const double n = (double)batch;
        const float pg = (float)(-s[0] / n), vfl = (float)(s[1] / n);
        const float ent = -((0.5f + 0.918938533204672742f) + theta[log_std_at]);
        stats[0] = pg;
        stats[1] = vfl;
        stats[2] = ent;
        stats[3] = (float)(s[2] / n);
        stats[4] = (float)(s[3] / n);
        stats[5] = (float)(s[4] / n);
        stats[6] = (float)(s[5] / n);
        stats[7] = (pg + ent_coef * ent) + vf_coef * vfl;
    }
