// b747_ppo_adv_stats_body.h -- the body of k_ppo_adv_stats and of its member-batched sibling k_pop_adv_stats
// (b747_ppo_update.h).  Textual, not an inlined function, as b747_eval_body.h: the existing kernel keeps its
// instruction stream.  In scope where it is included: POP, adv, idx, batch, part and pa (read with POP only).
// POP: member p = blockIdx.y works on its own perm row and its own slice of the workspace.
    if constexpr (POP) {
        idx += (int64_t)blockIdx.y * pa.n_rows;
        part = reinterpret_cast<double *>(reinterpret_cast<char *>(part) + (int64_t)blockIdx.y * pa.ws_stride);
    }
    __shared__ double red[2][256];
    const double x0 = (double)adv[upd_row<LOSS>(idx, 0)];
    double s = 0.0, q = 0.0;
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < batch; j += (int64_t)gridDim.x * 256) {
        const double d = (double)adv[upd_row<LOSS>(idx, j)] - x0;
        s += d;
        q += d * d;
    }
    red[0][threadIdx.x] = s;
    red[1][threadIdx.x] = q;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) {
            red[0][threadIdx.x] += red[0][threadIdx.x + w];
            red[1][threadIdx.x] += red[1][threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = red[0][0];
        part[2 * blockIdx.x + 1] = red[1][0];
    }
