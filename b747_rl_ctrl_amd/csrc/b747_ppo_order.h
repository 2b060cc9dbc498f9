// b747_ppo_order.h -- the minibatch sample orders of a population, drawn on the device in one launch
// (b747_ppo_sample_orders, include/b747.h).  The kernel lives in b747_ppo_order.hip; this is its
// launcher's declaration and the limits the entry point checks.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace b747 {

// One workgroup sorts one member's 64-bit keys in LDS: 8 bytes per key, padded to a power of two.  16,384 keys are
// 128 KiB of the CU's 160 KiB.
constexpr int32_t kOrderMaxRows = 16384;
constexpr int kOrderMaxBlock = 1024;     // threads per workgroup at most (fewer for fewer than 1,024 keys)
constexpr uint64_t kOrderTag = 0x6F72646572733A31ull;       // "orders:1": keeps the stream apart from the action noise
constexpr uint64_t kOrderFold = 0x9E3779B97F4A7C15ull;      // the fold of step_base's high word into the key

// Hidden: not part of the C ABI.  Arguments are validated by the caller: perm != NULL, n_policies >= 1, T >= 1,
// envs_per_policy a positive multiple of 64, n_policies * envs_per_policy <= N, T * envs_per_policy <= kOrderMaxRows.
__attribute__((visibility("hidden"))) hipError_t launch_ppo_sample_orders(int64_t *perm, int32_t n_policies, int32_t T,
                                                                          int32_t envs_per_policy, int64_t N,
                                                                          uint64_t seed, const uint64_t *step_base,
                                                                          uint32_t epoch, hipStream_t s);

}  // namespace b747
