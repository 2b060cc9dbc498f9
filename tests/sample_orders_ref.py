"""The reference of b747_ppo_sample_orders (include/b747.h), restated from the header's definition and
from nothing else: vectorised Philox4x32-10 on uint64 NumPy arrays, np.argsort(u, kind="stable"), the row mapping.
Shared by tests/test_ppo_sample_orders_abi.py (which checks it on the CPU against the scalar restatement below, plain
Python integers), tests/test_gpu_ppo_sample_orders.py and tests/test_gpu_ppo_population_device_order_train.py."""
import functools

import numpy as np

M32, M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
TAG, FOLD = 0x6F72646572733A31, 0x9E3779B97F4A7C15
MAX_ROWS = 16384


def order_key(seed: int, sb: int) -> int:
    """K = (seed ^ TAG) ^ ((sb >> 32) * FOLD), 64-bit wrap-around"""
    seed, sb = int(seed) & M64, int(sb) & M64
    return ((seed ^ TAG) ^ (((sb >> 32) * FOLD) & M64)) & M64


def philox4x32_10(key: int, c0, c1, c2, c3):
    """The four output words of Philox4x32-10 for every counter (c0, c1, c2, c3) (uint64 arrays of 32-bit values, or
    scalars that broadcast) under the 64-bit key: uint64 arrays of 32-bit values"""
    u = lambda x: np.asarray(x, dtype=np.uint64)
    m = np.uint64(M32)
    x0, x1, x2, x3 = np.broadcast_arrays(u(c0), u(c1), u(c2), u(c3))
    a, b = key & M32, (key >> 32) & M32
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * x0, np.uint64(0xCD9E8D57) * x2       # (32 x 32 bits: no overflow in uint64)
        x0, x1, x2, x3 = (p1 >> np.uint64(32)) ^ x1 ^ np.uint64(a), p1 & m, (p0 >> np.uint64(32)) ^ x3 ^ np.uint64(b), p0 & m
        a, b = (a + 0x9E3779B9) & M32, (b + 0xBB67AE85) & M32
    return x0, x1, x2, x3


def philox4x32_10_scalar(key: int, c0: int, c1: int, c2: int, c3: int):
    """The same block on plain Python integers, written out on its own (the check of the vectorised form)"""
    k0, k1 = key & M32, (key >> 32) & M32
    ctr = [c0 & M32, c1 & M32, c2 & M32, c3 & M32]
    for _ in range(10):
        hi0, lo0 = divmod(0xD2511F53 * ctr[0], 1 << 32)
        hi1, lo1 = divmod(0xCD9E8D57 * ctr[2], 1 << 32)
        ctr = [hi1 ^ ctr[1] ^ k0, lo1, hi0 ^ ctr[3] ^ k1, lo0]
        k0, k1 = (k0 + 0x9E3779B9) % (1 << 32), (k1 + 0xBB67AE85) % (1 << 32)
    return tuple(ctr)


def order_words(seed: int, sb: int, epoch: int, p: int, n_rows: int) -> np.ndarray:
    """u(p, l) for l < n_rows: word l & 3 of the block with counter (l >> 2, p, lo32(sb), epoch)"""
    l = np.arange(n_rows, dtype=np.uint64)
    words = np.stack(philox4x32_10(order_key(seed, sb), l >> np.uint64(2), p, (int(sb) & M64) & M32, int(epoch) & M32))
    return words[(l & np.uint64(3)).astype(np.int64), np.arange(n_rows)]


@functools.lru_cache(maxsize=None)
def local_order(seed: int, sb: int, epoch: int, p: int, n_rows: int) -> np.ndarray:
    """Member p's order of its own rows l = t * envs_per_policy + j (int64 [n_rows]; cached: do not modify)"""
    out = np.argsort(order_words(seed, sb, epoch, p, n_rows), kind="stable").astype(np.int64)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference_perm(P: int, T: int, epp: int, N: int, seed: int, sb: int, epoch: int) -> np.ndarray:
    """What b747_ppo_sample_orders writes: int64 [P, T * epp], the rows t * N + p * epp + j (cached: do not modify)"""
    out = np.empty((P, T * epp), dtype=np.int64)
    for p in range(P):
        l = local_order(seed, sb, epoch, p, T * epp)
        out[p] = (l // epp) * N + p * epp + l % epp
    out.setflags(write=False)
    return out
