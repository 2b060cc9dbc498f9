// b747_ppo_track.hip -- ControlTestCallback's bookkeeping (neural/callbacks.py:90-119) for every member of a population
// in one launch (b747_ppo_track.h): the kernel and its launcher, a translation unit of their own so that
// the kernels of the other units keep their generated code.
//
// All arithmetic is float64 in the order NumPy's np.mean of a list takes for up to 128 values (np_mean below), so the
// windowed means -- and with them every save decision -- are the callback's bit for bit given the same per-evaluation
// means.  No atomics; the same inputs give the same bits.
#include "b747_ppo_track.h"

#include <math.h>

namespace b747 {

namespace {

// np.mean of the n values a(0) .. a(n - 1) (NumPy's pairwise sum below its 128-value block: sequential under eight
// values, else eight running sums combined as a tree, then the n % 8 values left over, in order).  Checked bit for bit
// against NumPy for every n up to 128 (tests/test_ppo_track_best_abi.py); beyond 128 NumPy would split the range, this
// keeps the eight sums -- the entry point caps the window at 128, and more than 128 references are still a
// deterministic mean.
template <class F>
__device__ __forceinline__ double np_mean(int32_t n, F a)
{
    double s;
    if (n < 8) {
        s = 0.0;
        for (int32_t i = 0; i < n; ++i) s += a(i);
    } else {
        double r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = a(j);
        const int32_t full = n - n % 8;
        for (int32_t i = 8; i < full; i += 8) {
#pragma unroll
            for (int j = 0; j < 8; ++j) r[j] += a(i + j);
        }
        s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (int32_t i = full; i < n; ++i) s += a(i);
    }
    return s / (double)n;
}

}  // namespace

// One workgroup = one member p.
//   * All threads stage the member's three windows (ring[m][p][0 .. W)) in LDS.
//   * Lane m < 3 keeps metric m's books (0 settling_time, 1 |overshoot|, 2 quality): the mean over the member's n_refs
//     reported envs, then `repeat` pushes into its LDS window, the windowed mean after each; lane 2 also compares the
//     windowed quality with the best so far (strict >: a NaN never saves) and leaves the verdict in LDS.
//   * All threads write the windows back and, where the verdict says so, copy the member's parameter row to its
//     snapshot row, 16 bytes per lane and pass, consecutive lanes consecutive addresses.
// The uniform results (last, window_mean, count, best_quality, best_eval) are ordinary stores from the lane that
// computed them.
__global__ __launch_bounds__(kTrackBlock) void k_track_best(TrackArgs a)
{
    __shared__ double win[3][kTrackMaxWindow];
    __shared__ int32_t save;
    const uint32_t tid = threadIdx.x, p = blockIdx.x;
    const uint32_t W = (uint32_t)a.window, P = (uint32_t)a.n_members;

    for (uint32_t q = tid; q < 3u * W; q += kTrackBlock) {
        const uint32_t m = q / W, i = q - m * W;
        win[m][i] = a.ring[((int64_t)m * P + p) * W + i];
    }
    if (tid == 0) save = 0;
    __syncthreads();

    if (tid < 3u) {
        const uint32_t m = tid;
        const int64_t base = (int64_t)p * a.envs_per_policy;
        // eval_out's rows (B747_NEVAL): 0 overshoot, 2 settling_time, 4 itse
        const double *const src = a.eval_out + (int64_t)(m == 0u ? 2 : (m == 1u ? 0 : 4)) * a.n_eval + base;
        const double *const vr = a.vref + base;
        const double tk = a.tk;
        const double l = np_mean(a.n_refs, [&](int32_t i) -> double {
            const double x = src[i];
            if (m == 0u) return x;
            if (m == 1u) return fabs(x);
            const double v = vr[i];
            return exp(-60 * 0.1 * x / (tk * (v * v)));      // Controller.quality, evaluate.quality
        });
        a.last[(int64_t)p * 3 + m] = l;

        int64_t cnt = a.count[p];
        double wm = l, bq = a.best_quality[p];
        int64_t be = a.best_eval[p];
        bool sv = false;
        for (int32_t r = 0; r < a.repeat; ++r) {
            win[m][(uint32_t)(cnt % (int64_t)W)] = l;
            ++cnt;
            const bool wrapped = cnt >= (int64_t)W;
            const int32_t nw = wrapped ? (int32_t)W : (int32_t)cnt;
            const uint32_t oldest = wrapped ? (uint32_t)(cnt % (int64_t)W) : 0u;
            wm = np_mean(nw, [&](int32_t i) -> double {
                uint32_t j = oldest + (uint32_t)i;
                if (j >= W) j -= W;
                return win[m][j];
            });
            if (m == 2u && wm > bq) {
                bq = wm;
                be = cnt - 1;
                sv = true;
            }
        }
        a.window_mean[(int64_t)p * 3 + m] = wm;
        if (m == 2u) {
            a.count[p] = cnt;
            a.best_quality[p] = bq;
            a.best_eval[p] = be;
            if (sv) save = 1;
        }
    }
    __syncthreads();

    for (uint32_t q = tid; q < 3u * W; q += kTrackBlock) {
        const uint32_t m = q / W, i = q - m * W;
        a.ring[((int64_t)m * P + p) * W + i] = win[m][i];
    }
    if (save) {
        const float4 *const from = reinterpret_cast<const float4 *>(a.params + (int64_t)p * a.stride);
        float4 *const to = reinterpret_cast<float4 *>(a.best_params + (int64_t)p * a.stride);
        const int64_t n4 = a.stride / 4;
        for (int64_t q = tid; q < n4; q += kTrackBlock) to[q] = from[q];
    }
}

hipError_t launch_ppo_track_best(const TrackArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(k_track_best, dim3((unsigned)a.n_members), dim3(kTrackBlock), 0, s, a);
    return hipGetLastError();
}

}  // namespace b747
