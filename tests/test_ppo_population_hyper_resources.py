"""Register use of the kernels that read per-member hyper-parameters from a device table (k_hyp_grad<obs_dim>,
k_hyp_reduce, k_hyp_adam, csrc/b747_ppo_update.h; k_pop_gae, csrc/b747_ppo_gae.hip), read on the CPU from
the shipped gfx950 code object (as tests/test_ppo_epoch_batched_resources.py).  Each is an existing kernel's text behind
a few loads from its member's table row: workgroup-uniform values that belong in SGPRs, so no scratch, no spills, and
k_hyp_grad<obs_dim> within the 8 registers above k_pop_grad<obs_dim> that a member offset is allowed."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "b747_rl_ctrl_amd", "libb747.so")
pytestmark = pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"),
                                reason="needs the built library and the ROCm LLVM tools")


def test_hyper_table_kernels_fit_the_register_file_beside_the_kernels_whose_text_they_run():
    import kernel_resources
    res = kernel_resources.resources(LIB)
    regs = lambda x: x["vgpr_count"] + x["agpr_count"]   # (vgpr_count is the unified file's total: an upper bound)
    grad = {n: f for n, f in res.items() if "k_hyp_grad<" in n}
    assert len(grad) == 5, sorted(grad)                      # obs_dim 3, 5, 7, 8, 10
    reduce_ = {n: f for n, f in res.items() if "k_hyp_reduce" in n}
    adam = {n: f for n, f in res.items() if "k_hyp_adam" in n}
    gae = {n: f for n, f in res.items() if "k_pop_gae" in n}
    assert len(reduce_) == 1 and len(adam) == 1 and len(gae) == 1, (sorted(reduce_), sorted(adam), sorted(gae))
    for name, f in {**grad, **reduce_, **adam, **gae}.items():
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0, (name, f)
        assert f["vgpr_count"] <= 512 and regs(f) <= 512, (name, f)
    pop = {int(re.search(r"k_pop_grad<(\d+)>", n).group(1)): f for n, f in res.items() if "k_pop_grad<" in n}
    assert sorted(pop) == [3, 5, 7, 8, 10]
    for name, f in grad.items():
        od = int(re.search(r"k_hyp_grad<(\d+)>", name).group(1))
        print(f"k_hyp_grad<{od}> vgpr {f['vgpr_count']} agpr {f['agpr_count']}; k_pop_grad<{od}> vgpr "
              f"{pop[od]['vgpr_count']} agpr {pop[od]['agpr_count']}")
        assert regs(f) <= regs(pop[od]) + 8, (name, f, pop[od])
    # the population GAE kernel holds what k_ppo_gae<16> holds: at least two waves per SIMD
    single = [f for n, f in res.items() if "k_ppo_gae<" in n]
    assert len(single) == 1
    for name, f in gae.items():
        print(f"{name.split('(')[0]} vgpr {f['vgpr_count']}; k_ppo_gae vgpr {single[0]['vgpr_count']}")
        assert f["vgpr_count"] <= 256, (name, f)


def test_the_kernel_counts_of_the_older_resource_tests_are_what_they_were():
    """(their name filters must not catch the new kernels: 1 GAE kernel, 5 + 3 single-member and 5 + 3 member-batched
    update kernels)"""
    import kernel_resources
    res = kernel_resources.resources(LIB)
    count = lambda *keys: sum(any(k in n for k in keys) for n in res)
    assert count("k_ppo_gae<") == 1
    assert count("k_ppo_grad<") == 5 and count("k_ppo_adv_stats", "k_ppo_reduce", "k_ppo_adam") == 3
    assert count("k_pop_grad<") == 5 and count("k_pop_adv_stats", "k_pop_reduce", "k_pop_adam") == 3
