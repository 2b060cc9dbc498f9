"""b747_ppo_sample_orders on the GPU (include/b747.h) against the NumPy restatement of its definition
(tests/sample_orders_ref.py: Philox4x32-10 on uint64, a stable argsort, the row mapping).  The keys are distinct
integers, so every correct sort gives the reference's order: exact equality, no tolerance.

Shapes (P, T, envs_per_policy, N): one wave with nothing padded; fewer keys than the workgroup has threads, padded;
several keys per thread, padded, and more envs than the members hold; 8,192 rows; 16,384 rows, the limit (128 KiB of
LDS, the dynamic limit raised)."""
import numpy as np
import pytest
import torch

import sample_orders_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 64, 64), (3, 5, 64, 192), (2, 17, 64, 200), (2, 64, 128, 256), (2, 256, 64, 128)]
# ... and the smallest sizes at which the sort has a step through LDS: 128 keys (one such step, nothing padded) and 192
# rows padded to 256 (three, the runs of 128 descending in the upper half)
EDGE_SHAPES = [(1, 2, 64, 64), (2, 3, 64, 128)]
SEED, SB, EPOCH = 11, 7, 1
BIG_SEED, BIG_SB = (1 << 40) + 12345, (1 << 32) + 7
GUARD, SENTINEL = 64, -0x0123456789ABCDEF


class _Call:
    """perm between two rows of guard words, and step_base, on the device"""

    def __init__(self, P, T, epp, N, sb=SB):
        self.shape, self.n = (P, T, epp, N), P * T * epp
        self.buf = torch.full((GUARD + self.n + GUARD,), SENTINEL, dtype=torch.int64, device="cuda")
        self.sb = None if sb is None else torch.tensor([sb], dtype=torch.int64, device="cuda")

    def __call__(self, seed=SEED, epoch=EPOCH):
        from b747_rl_ctrl_amd import _lib
        P, T, epp, N = self.shape
        _lib.check(_lib.lib().b747_ppo_sample_orders(
            self.buf.data_ptr() + 8 * GUARD, P, T, epp, N, seed, None if self.sb is None else self.sb.data_ptr(), epoch,
            torch.cuda.current_stream().cuda_stream), "b747_ppo_sample_orders")
        return self

    def perm(self) -> np.ndarray:
        P, T, epp, _ = self.shape
        torch.cuda.synchronize()
        host = self.buf.cpu()
        assert bool((host[:GUARD] == SENTINEL).all()) and bool((host[GUARD + self.n:] == SENTINEL).all()), \
            "guard words around perm were written"
        return host[GUARD:GUARD + self.n].view(P, T * epp).numpy()


def _same(got, ref, what):
    bad = np.argwhere(got != ref)
    assert bad.size == 0, f"{what}: {len(bad)} of {got.size} entries differ, the first at {tuple(bad[0])}: " \
                          f"{got[tuple(bad[0])]} for {ref[tuple(bad[0])]}"


@pytest.mark.parametrize("shape", SHAPES + EDGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_perm_is_the_reference_and_the_guard_words_stay(shape):
    _same(_Call(*shape)().perm(), R.reference_perm(*shape, SEED, SB, EPOCH), str(shape))


@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[4]], ids=lambda s: "x".join(map(str, s)))
def test_both_64_bit_folds(shape):
    """step_base = 2^32 + 7 (its high word reaches the key, its low word the counter) and a seed above 2^32"""
    _same(_Call(*shape, sb=BIG_SB)(seed=BIG_SEED, epoch=9).perm(), R.reference_perm(*shape, BIG_SEED, BIG_SB, 9),
          str(shape))
    assert not np.array_equal(R.reference_perm(*shape, BIG_SEED, BIG_SB, 9), R.reference_perm(*shape, BIG_SEED, 7, 9))
    assert not np.array_equal(R.reference_perm(*shape, BIG_SEED, BIG_SB, 9), R.reference_perm(*shape, 12345, BIG_SB, 9))


def test_a_null_step_base_is_step_base_zero():
    shape = SHAPES[1]
    _same(_Call(*shape, sb=None)().perm(), R.reference_perm(*shape, SEED, 0, EPOCH), "NULL step_base")
    _same(_Call(*shape, sb=0)().perm(), R.reference_perm(*shape, SEED, 0, EPOCH), "step_base 0")


def test_two_calls_with_equal_inputs_are_equal_and_every_input_changes_the_order():
    shape = SHAPES[2]
    P, T, epp, N = shape
    base = _Call(*shape)().perm()
    _same(_Call(*shape)().perm(), base, "a second buffer")
    call = _Call(*shape)
    _same(call()().perm(), base, "the same buffer twice")
    local = lambda perm, p: perm[p] - p * epp                  # (member p's order as member 0 would hold it)
    assert not np.array_equal(local(base, 0), local(base, 1)), "member"
    for what, other in (("epoch", _Call(*shape)(epoch=EPOCH + 1)), ("seed", _Call(*shape)(seed=SEED + 1)),
                        ("step_base", _Call(*shape, sb=SB + 1)()), ("step_base's high word", _Call(*shape, sb=SB + (1 << 32))())):
        got = other.perm()
        for p in range(P):
            assert not np.array_equal(got[p], base[p]), (what, p)
            assert np.array_equal(np.sort(got[p]), np.sort(base[p])), (what, p)


def test_one_captured_graph_draws_fresh_orders_after_step_base_changes_on_the_device():
    shape = SHAPES[2]
    call = _Call(*shape)
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=s):          # (the capture launches nothing)
        call()
    torch.cuda.synchronize()
    assert bool((call.buf == SENTINEL).all())
    g.replay()
    _same(call.perm(), R.reference_perm(*shape, SEED, SB, EPOCH), "the first replay")
    call.sb.add_(17)                             # what a rollout of 17 steps does
    g.replay()
    _same(call.perm(), R.reference_perm(*shape, SEED, SB + 17, EPOCH), "the replay after step_base moved")
    call.sb.fill_(BIG_SB)
    g.replay()
    _same(call.perm(), R.reference_perm(*shape, SEED, BIG_SB, EPOCH), "the replay after step_base's high word moved")


def test_the_limit_is_refused_on_the_device_too():
    from b747_rl_ctrl_amd import _lib
    call = _Call(1, 1, 64, 64)
    rc = _lib.lib().b747_ppo_sample_orders(call.buf.data_ptr() + 8 * GUARD, 1, 257, 64, 64, SEED, call.sb.data_ptr(), 0,
                                           torch.cuda.current_stream().cuda_stream)
    assert rc == -1 and b"T * envs_per_policy > 16384" in _lib.lib().b747_last_error()
    torch.cuda.synchronize()
    assert bool((call.buf == SENTINEL).all())
