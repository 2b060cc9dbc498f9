"""Register use of the GAE kernel (k_ppo_gae, csrc/b747_ppo_gae.hip), read on the CPU from the shipped gfx950 code
object (as tests/test_ppo_update_resources.py).  A lane holds two chunks of U rows (three loads per row) beside the
recurrence: that must fit the register file with no scratch and no VGPR spills."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "b747_rl_ctrl_amd", "libb747.so")
pytestmark = pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"),
                                reason="needs the built library and the ROCm LLVM tools")


def test_gae_kernel_has_no_scratch_and_no_vgpr_spills():
    import kernel_resources
    res = kernel_resources.resources(LIB)
    gae = {n: f for n, f in res.items() if "k_ppo_gae<" in n}
    assert len(gae) == 1, sorted(gae)                        # one instantiation: the shipped unroll factor
    for name, f in gae.items():
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0, (name, f)
        # two chunks of 16 rows x 3 values and their addresses; at least two waves per SIMD (512 registers) must fit,
        # so that one wave's stores overlap another's loads when there are more envs than SIMDs
        assert f["vgpr_count"] <= 256, (name, f)
