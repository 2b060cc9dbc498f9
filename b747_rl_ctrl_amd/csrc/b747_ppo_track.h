// b747_ppo_track.h -- the reference's ControlTestCallback kept on the device: the windows of the last step-test
// evaluations, the best windowed quality so far and a snapshot of the parameters that reached it, for every member of
// a population in one launch (b747_ppo_track_best, include/b747.h).  The kernel lives in
// b747_ppo_track.hip; this is its launcher's declaration and the limits the entry point checks.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace b747 {

constexpr int kTrackBlock = 256;              // threads per workgroup: three of them keep the books, all of them copy
constexpr int32_t kTrackMaxWindow = 128;      // NumPy sums up to 128 values with eight accumulators and no split
constexpr int32_t kTrackMaxRepeat = 256;      // pushes of one evaluation per call at most

struct TrackArgs {
    const double *eval_out;   // [B747_NEVAL][n_eval]
    const double *vref;       // [n_eval]
    const float *params;      // [n_members][stride]
    double *ring;             // [3][n_members][window]
    int64_t *count;           // [n_members]
    double *last;             // [n_members][3]
    double *window_mean;      // [n_members][3]
    double *best_quality;     // [n_members]
    int64_t *best_eval;       // [n_members]
    float *best_params;       // [n_members][stride]
    int64_t n_eval, stride;
    double tk;
    int32_t n_members, envs_per_policy, n_refs, window, repeat;
};

// Hidden: not part of the C ABI.  Arguments are validated by the caller (b747_ppo_track_best's refusals).
__attribute__((visibility("hidden"))) hipError_t launch_ppo_track_best(const TrackArgs &a, hipStream_t s);

}  // namespace b747
