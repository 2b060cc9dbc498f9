// b747_ppo_adam_body.h -- the body of k_ppo_adam and of its member-batched sibling k_pop_adam (b747_ppo_update.h).
// Textual, not an inlined function, as b747_eval_body.h: the existing kernel keeps its instruction stream.  In scope
// where it is included: POP, the arguments of k_ppo_adam (lr a double: k_pop_adam loads its member's from the device
// array before the body) and pa (read with POP only).
// POP: member p = blockIdx.y updates its own parameters, moments and step count from the gradient vector of its
// workspace slice.
    if constexpr (POP) {
        theta += (int64_t)blockIdx.y * pa.policy_stride;
        m += (int64_t)blockIdx.y * pa.n_params;
        v += (int64_t)blockIdx.y * pa.n_params;
        t += blockIdx.y;
        grad = reinterpret_cast<const float *>(reinterpret_cast<const char *>(grad) + (int64_t)blockIdx.y * pa.ws_stride);
    }
    __shared__ double red[kUpdAdamBlock];
    const int tid = threadIdx.x;
    const int64_t step = t[0] + 1;
    double q = 0.0;
    for (int64_t i = tid; i < n; i += kUpdAdamBlock) {
        const double g = (double)(float)(grad_scale * (double)grad[i]);
        q += g * g;
    }
    red[tid] = q;
    __syncthreads();
    for (int w = kUpdAdamBlock / 2; w >= 1; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    const double norm = sqrt(red[0]);
    const double c0 = max_norm / (norm + 1e-6), coef = c0 < 1.0 ? c0 : 1.0;
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2s = sqrt(1.0 - pow(beta2, (double)step));
    const double step_size = lr / bc1;
    for (int64_t i = tid; i < n; i += kUpdAdamBlock) {
        const double g = (double)(float)((double)(float)(grad_scale * (double)grad[i]) * coef);
        const double mi = (double)m[i] + (1.0 - beta1) * (g - (double)m[i]);
        const double vi = beta2 * (double)v[i] + (1.0 - beta2) * g * g;
        const float mf = (float)mi, vf = (float)vi;
        m[i] = mf;
        v[i] = vf;
        theta[i] = (float)((double)theta[i] - step_size * ((double)mf / (sqrt((double)vf) / bc2s + eps)));
    }
    if (tid == 0) t[0] = step;   // (every thread read the old count before the first barrier)
