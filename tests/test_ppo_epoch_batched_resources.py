"""Register use of the member-batched PPO update kernels (k_pop_*, csrc/b747_ppo_update.h), read on the
CPU from the shipped gfx950 code object (as tests/test_ppo_update_resources.py).  k_pop_grad<obs_dim> is
k_ppo_grad<obs_dim>'s text behind a member offset: one wave per SIMD with the whole register file, no scratch, no
spills, and at most 8 registers above its single-member kernel (the population forms of DESIGN.md 13 and 14 cost 2;
the offsets are workgroup-uniform and belong in SGPRs)."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "b747_rl_ctrl_amd", "libb747.so")
pytestmark = pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"),
                                reason="needs the built library and the ROCm LLVM tools")


def test_batched_update_kernels_fit_the_register_file_beside_their_single_member_kernels():
    import kernel_resources
    res = kernel_resources.resources(LIB)
    grad = {n: f for n, f in res.items() if "k_pop_grad<" in n}
    assert len(grad) == 5, sorted(grad)                      # obs_dim 3, 5, 7, 8, 10
    small = {n: f for n, f in res.items() if any(k in n for k in ("k_pop_adv_stats", "k_pop_reduce", "k_pop_adam"))}
    assert len(small) == 3, sorted(small)
    for name, f in {**grad, **small}.items():
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0, (name, f)
    single = {int(re.search(r"k_ppo_grad<(\d+)>", n).group(1)): f for n, f in res.items() if "k_ppo_grad<" in n}
    assert sorted(single) == [3, 5, 7, 8, 10]
    for name, f in grad.items():
        od = int(re.search(r"k_pop_grad<(\d+)>", name).group(1))
        # (the metadata's vgpr_count is the unified file's total, AGPRs included: the sum is an upper bound)
        regs = lambda x: x["vgpr_count"] + x["agpr_count"]
        print(f"k_pop_grad<{od}> vgpr {f['vgpr_count']} agpr {f['agpr_count']}; k_ppo_grad<{od}> vgpr "
              f"{single[od]['vgpr_count']} agpr {single[od]['agpr_count']}")
        assert f["vgpr_count"] <= 512 and regs(f) <= 512, (name, f)
        assert regs(f) <= regs(single[od]) + 8, (name, f, single[od])
