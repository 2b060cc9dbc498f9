// b747_ppo_gae_body.h -- the body of k_ppo_gae<U> and of its population sibling k_pop_gae<U> (b747_ppo_gae.hip).
// Textual, not an inlined function, as b747_ppo_grad_body.h: the existing kernel keeps its instruction stream.  In
// scope where it is included: U, the arguments of k_ppo_gae (g and gl floats: k_pop_gae computes them from its
// member's table row before the body).
    const int64_t i = (int64_t)blockIdx.x * kGaeBlock + threadIdx.x;
    const bool live = i < N;
    const int64_t col = live ? i : N - 1;
    float nv = last_value[col], a = 0.0f;
    int32_t t = T - 1;
    GaeRows<U> cur, nxt;
    gae_load<U>(cur, rew, val, done, t, N, col);
#pragma unroll 1
    for (;;) {
        const int32_t tn = t - U;
        if (tn >= 0) gae_load<U>(nxt, rew, val, done, tn, N, col);
        if (t >= U - 1) gae_steps<U, false>(cur, t, N, col, live, g, gl, nv, a, adv, ret);
        else gae_steps<U, true>(cur, t, N, col, live, g, gl, nv, a, adv, ret);
        if (tn < 0) break;
        cur = nxt;
        t = tn;
    }
