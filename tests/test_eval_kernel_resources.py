"""Register use of the evaluation-episode kernels, read on the CPU from the shipped gfx950 code object (as
tests/test_kernel_resources.py): k_eval_episodes runs one wave per 64-lane workgroup so that the wave has the whole
register file -- the env lane, the RK4 stage and the policy head's matrix-core tiles together.  The FAST
instantiations (no policy, obs_dim 3, obs_dim 5) must fit it: no scratch and no VGPR spills.  (FAITHFUL is reported
in DESIGN.md, not gated.)"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "b747_rl_ctrl_amd", "libb747.so")
pytestmark = pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"),
                                reason="needs the built library and the ROCm LLVM tools")


def test_fast_eval_kernels_have_no_scratch_and_no_vgpr_spills():
    import kernel_resources
    res = kernel_resources.resources(LIB)
    got = {n: f for n, f in res.items() if "k_eval_episodes<" in n}
    assert len(got) == 6, sorted(got)            # FAST / FAITHFUL x (no policy, obs_dim 3, obs_dim 5)
    fast = {n: f for n, f in got.items() if "k_eval_episodes<true" in n}
    assert len(fast) == 3, sorted(fast)
    for name, f in fast.items():
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0, (name, f)
