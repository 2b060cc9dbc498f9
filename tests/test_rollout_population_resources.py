"""Register and LDS use of the population PPO rollout kernels (k_rollout_population, csrc/b747_rollout_population.h),
read on the CPU from the shipped gfx950 code object (as tests/test_rollout_lanes_resources.py).  Eight instantiations:
FAST / FAITHFUL x (obs_dim 3, obs_dim 5) x (the batch's reward constants, a row per group).  Every FAST one must fit the
wave's register file (no scratch, no VGPR spills) and every one must stay at or below 40 KB of LDS, so that four
workgroups still share a CU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "b747_rl_ctrl_amd", "libb747.so")
pytestmark = pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"),
                                reason="needs the built library and the ROCm LLVM tools")
WANT = {f"k_rollout_population<{fast}, {od}, {rew}>" for fast in ("true", "false") for od in (3, 5)
        for rew in ("false", "true")}


@pytest.fixture(scope="module")
def population_kernels():
    import kernel_resources
    res = kernel_resources.resources(LIB)
    got = {n: f for n, f in res.items() if "k_rollout_population<" in n}
    short = {n[n.index("k_rollout_population<"):n.index(">") + 1]: f for n, f in got.items()}
    assert len(got) == 8 and set(short) == WANT, sorted(got)
    return short


def test_fast_rollout_population_kernels_have_no_scratch_and_no_vgpr_spills(population_kernels):
    fast = {n: f for n, f in population_kernels.items() if n.startswith("k_rollout_population<true")}
    assert len(fast) == 4, sorted(fast)
    for name, f in fast.items():
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0, (name, f)


def test_every_rollout_population_kernel_keeps_four_workgroups_per_cu(population_kernels):
    for name, f in population_kernels.items():
        print(name, {k: f[k] for k in ("vgpr_count", "agpr_count", "sgpr_spill_count", "vgpr_spill_count",
                                       "private_segment_fixed_size", "group_segment_fixed_size")})
        assert f["group_segment_fixed_size"] <= 40 * 1024, (name, f)


def test_the_population_kernels_do_not_count_as_rollout_lanes_kernels(population_kernels):
    """tests/test_rollout_lanes_resources.py counts the four k_rollout_lanes instantiations by that substring"""
    import kernel_resources
    res = kernel_resources.resources(LIB)
    assert sum("k_rollout_lanes<" in n for n in res) == 4
    assert not any("k_rollout_lanes<" in n for n in res if "k_rollout_population<" in n)
