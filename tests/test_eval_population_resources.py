"""Register and LDS use of the population evaluation kernels (k_eval_population, csrc/b747_eval.h), read on the CPU from
the shipped gfx950 code object (as tests/test_eval_kernel_resources.py).  Ten instantiations: FAST / FAITHFUL x
(obs_dim 3, obs_dim 5) x (batch gains, per-env gains) and FAST / FAITHFUL x (no policy, per-env gains); no policy with
batch gains is k_eval_episodes<*, 0> itself.  Every FAST one must fit the wave's register file (no scratch, no VGPR
spills) and every one must stay at or below 40 KB of LDS, so that four workgroups still share a CU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "b747_rl_ctrl_amd", "libb747.so")
pytestmark = pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"),
                                reason="needs the built library and the ROCm LLVM tools")
WANT = {f"k_eval_population<{fast}, {od}, {gains}>" for fast in ("true", "false")
        for od, gains in ((3, "false"), (3, "true"), (5, "false"), (5, "true"), (0, "true"))}


@pytest.fixture(scope="module")
def population_kernels():
    import kernel_resources
    res = kernel_resources.resources(LIB)
    got = {n: f for n, f in res.items() if "k_eval_population<" in n}
    short = {n[n.index("k_eval_population<"):n.index(">") + 1]: f for n, f in got.items()}
    assert set(short) == WANT, sorted(short)
    return short


def test_fast_population_kernels_have_no_scratch_and_no_vgpr_spills(population_kernels):
    fast = {n: f for n, f in population_kernels.items() if n.startswith("k_eval_population<true")}
    assert len(fast) == 5, sorted(fast)
    for name, f in fast.items():
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0, (name, f)


def test_every_population_kernel_keeps_four_workgroups_per_cu(population_kernels):
    for name, f in population_kernels.items():
        print(name, {k: f[k] for k in ("vgpr_count", "agpr_count", "sgpr_spill_count", "vgpr_spill_count",
                                       "private_segment_fixed_size", "group_segment_fixed_size")})
        assert f["group_segment_fixed_size"] <= 40 * 1024, (name, f)


def test_the_batched_pack_kernel_is_there():
    import kernel_resources
    assert any("k_policy_pack_batch" in n for n in kernel_resources.resources(LIB))
