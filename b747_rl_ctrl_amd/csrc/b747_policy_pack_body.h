// b747_policy_pack_body.h -- the body of k_policy_pack / k_policy_pack_batch (b747_policy.h), included by both:
// one thread per packed half-element, then one per derived float, then one per layer-1 fragment half.  In scope:
// params (the policy's own buffer) and od.  (Textual for the reason given in b747_eval_body.h.)
    const PolicyLayout L = PolicyLayout::of(od);
    const PolicyDerived D = PolicyDerived::of(od);
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int l1i = idx - (4 * kPackPerHead + D.total);
    if (l1i >= 0) {   // layer-1 A fragments (policy_l1pack_offset): half ((head * 2 + mt) * 64 + lane) * 8 + j
        if (l1i >= 2 * kL1PackFloats) return;
        const int j = l1i & 7, lane = (l1i >> 3) & 63, frag = l1i >> 9, mt = frag & 1, head = frag >> 1;
        const int u = mt * 32 + (lane & 31), k = 8 * (lane >> 5) + j;
        const int w1 = head ? L.vf_w1 : L.pi_w1, b1 = head ? L.vf_b1 : L.pi_b1;
        auto split = [](float x, bool lo) {
            const _Float16 h = (_Float16)x;
            return lo ? (_Float16)(x - (float)h) : h;
        };
        _Float16 v = (_Float16)0.0f;
        if (od <= kL1MaxOD) {
            if (k < 2 * od) v = split(kTanhScale * params[w1 + u * od + (k % od)], false);       // hi, hi
            else if (k < 3 * od) v = split(kTanhScale * params[w1 + u * od + (k - 2 * od)], true);  // lo
            else if (k == 3 * od) v = split(kTanhScale * params[b1 + u], false);
            else if (k == 3 * od + 1) v = split(kTanhScale * params[b1 + u], true);
        }
        reinterpret_cast<_Float16 *>(params + policy_l1pack_offset(od))[l1i] = v;
        return;
    }
    if (idx < 2 * 2 * kPackPerHead) {
        const int head = idx / (2 * kPackPerHead), rem = idx % (2 * kPackPerHead);
        const int j = rem & 7, lane = (rem >> 3) & 63, frag = rem >> 9;  // frag = (mt*4 + s)*2 + part
        const int part = frag & 1, s = (frag >> 1) & 3, mt = frag >> 3;
        const int w2 = head ? L.vf_w2 : L.pi_w2;
        const float x = -2.0f * kTanhScale * params[w2 + (mt * 32 + (lane & 31)) * PH + 16 * s + 8 * (lane >> 5) + j];
        const _Float16 hi = (_Float16)x;
        const _Float16 v = part ? (_Float16)(x - (float)hi) : hi;
        reinterpret_cast<_Float16 *>(params + policy_packed_offset(od) + head * kPackPerHead)[rem] = v;
        return;
    }
    const int d = idx - 2 * 2 * kPackPerHead;
    if (d >= D.total) return;
    float v;
    if (d < D.acc0) {
        const int head = d / (PH * (od + 1)), rem = d % (PH * (od + 1)), j = rem / (od + 1), k = rem % (od + 1);
        const int w1 = head ? L.vf_w1 : L.pi_w1, b1 = head ? L.vf_b1 : L.pi_b1;
        v = kTanhScale * (k < od ? params[w1 + j * od + k] : params[b1 + j]);
    } else if (d < D.hw) {
        const int head = (d - D.acc0) / PH, row = (d - D.acc0) % PH;
        const int w2 = head ? L.vf_w2 : L.pi_w2, b2 = head ? L.vf_b2 : L.pi_b2;
        float a = params[b2 + row];
        for (int k = 0; k < PH; ++k) a += params[w2 + row * PH + k];
        v = kTanhScale * a;
    } else if (d < D.c) {
        const int head = (d - D.hw) / PH, row = (d - D.hw) % PH;
        v = -2.0f * params[(head ? L.wv : L.wa) + row];
    } else if (d < D.log_std) {
        const int head = d - D.c;
        float a = params[head ? L.bv : L.ba];
        for (int k = 0; k < PH; ++k) a += params[(head ? L.wv : L.wa) + k];
        v = a;
    } else {
        v = params[L.log_std];
    }
    params[policy_derived_offset(od) + d] = v;
