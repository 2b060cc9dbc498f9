"""Register use of the one-wave PPO rollout kernels, read on the CPU from the shipped gfx950 code object (as
tests/test_eval_kernel_resources.py): k_rollout_lanes runs one wave per 64-lane workgroup so that the wave has the
whole register file -- the env lane, the RK4 stage and both policy heads' matrix-core tiles together.  The FAST
instantiations (obs_dim 3, obs_dim 5) must fit it: no scratch and no VGPR spills.  (FAITHFUL is reported in
DESIGN.md 12, not gated.)"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "b747_rl_ctrl_amd", "libb747.so")
pytestmark = pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"),
                                reason="needs the built library and the ROCm LLVM tools")


def test_fast_rollout_lanes_kernels_have_no_scratch_and_no_vgpr_spills():
    import kernel_resources
    res = kernel_resources.resources(LIB)
    got = {n: f for n, f in res.items() if "k_rollout_lanes<" in n}
    assert len(got) == 4, sorted(got)            # FAST / FAITHFUL x (obs_dim 3, obs_dim 5)
    fast = {n: f for n, f in got.items() if "k_rollout_lanes<true" in n}
    assert len(fast) == 2, sorted(fast)
    for name, f in fast.items():
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0, (name, f)


def test_four_workgroups_of_the_rollout_lanes_kernel_fit_a_cu():
    """160 KB of LDS per CU: at or below 40 KB a workgroup, four one-wave workgroups (one per SIMD) are resident, and
    65,536 envs (1,024 waves on 256 CUs) run in one round (the evaluation kernel's measurement, csrc/b747_eval.h)"""
    import kernel_resources
    res = kernel_resources.resources(LIB)
    for name, f in res.items():
        if "k_rollout_lanes<" in name:
            assert f["group_segment_fixed_size"] <= 40 * 1024, (name, f)
