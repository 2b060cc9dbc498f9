"""Register use of the fused PPO update's kernels, read on the CPU from the shipped gfx950 code object (as
tests/test_eval_kernel_resources.py).  k_ppo_grad<obs_dim> runs one wave per SIMD (256 threads per workgroup, one
workgroup per CU) so that a wave has the whole register file for one net's gradient accumulators (the 64x64 dW2
as four matrix-core tiles) beside the tile's activations: every instantiation must fit it with no scratch and no
VGPR spills, and so must the three small kernels around it."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "b747_rl_ctrl_amd", "libb747.so")
pytestmark = pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"),
                                reason="needs the built library and the ROCm LLVM tools")


def test_update_kernels_have_no_scratch_and_no_vgpr_spills():
    import kernel_resources
    res = kernel_resources.resources(LIB)
    grad = {n: f for n, f in res.items() if "k_ppo_grad<" in n}
    assert len(grad) == 5, sorted(grad)                      # obs_dim 3, 5, 7, 8, 10
    small = {n: f for n, f in res.items() if any(k in n for k in ("k_ppo_adv_stats", "k_ppo_reduce", "k_ppo_adam"))}
    assert len(small) == 3, sorted(small)
    for name, f in {**grad, **small}.items():
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0, (name, f)
    for name, f in grad.items():                             # the unified register file of one wave per SIMD
        assert f["vgpr_count"] <= 512, (name, f)
