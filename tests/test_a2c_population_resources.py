"""Register use of the member-batched A2C update kernels (k_apop_*, csrc/b747_a2c_population.hip), read on
the CPU from the shipped gfx950 code object (as tests/test_ppo_epoch_batched_resources.py).  k_apop_grad<obs_dim> is
k_a2c_grad<obs_dim>'s text behind a member offset: no scratch, no spills, and at most 8 registers above its
single-member kernel (the allowance tests/test_ppo_epoch_batched_resources.py gives a member offset: the offsets are
workgroup-uniform and belong in SGPRs) -- a condition, not a measurement.  The families that were there keep their
counts."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "b747_rl_ctrl_amd", "libb747.so")
pytestmark = pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"),
                                reason="needs the built library and the ROCm LLVM tools")
OBS_DIMS = [3, 5, 7, 8, 10]
SMALL = ("k_apop_adv_stats", "k_apop_reduce", "k_apop_opt")
# what every family had before this one: the templated ones by their opening bracket, the others by name
FAMILIES = {"k_ppo_grad<": 5, "k_pop_grad<": 5, "k_hyp_grad<": 5, "k_a2c_grad<": 5, "k_ppo_adv_stats": 1,
            "k_pop_adv_stats": 1, "k_a2c_adv_stats": 1, "k_ppo_reduce": 1, "k_pop_reduce": 1, "k_hyp_reduce": 1,
            "k_a2c_reduce": 1, "k_ppo_adam": 1, "k_pop_adam": 1, "k_hyp_adam": 1, "k_ppo_rmsprop": 1, "k_ppo_gae<": 1,
            "k_pop_gae": 1}


def _resources():
    import kernel_resources
    return kernel_resources.resources(LIB)


def _by_obs_dim(res, kernel):
    out = {}
    for name, f in res.items():
        m = re.search(kernel + r"<(\d+)>", name)
        if m:
            assert int(m.group(1)) not in out, name
            out[int(m.group(1))] = f
    return out


def test_the_population_kernels_exist_once_each():
    res = _resources()
    assert sorted(_by_obs_dim(res, "k_apop_grad")) == OBS_DIMS
    for k in SMALL:
        assert len([n for n in res if k in n]) == 1, k


def test_no_scratch_and_no_spills_of_either_kind():
    res = _resources()
    grad = {f"k_apop_grad<{od}>": f for od, f in _by_obs_dim(res, "k_apop_grad").items()}
    small = {n: f for n, f in res.items() if any(k in n for k in SMALL)}
    assert len(grad) == 5 and len(small) == 3
    for name, f in {**grad, **small}.items():
        print(f"{name.split('(')[0]}: vgpr {f['vgpr_count']} agpr {f['agpr_count']} sgpr {f['sgpr_count']} "
              f"sgpr spills {f['sgpr_spill_count']}")
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0, (name, f)
        assert (f["sgpr_spill_count"] or 0) == 0, (name, f)
        assert f["vgpr_count"] + f["agpr_count"] <= 512, (name, f)


def test_the_member_offset_costs_at_most_8_registers():
    res = _resources()
    pop, single = _by_obs_dim(res, "k_apop_grad"), _by_obs_dim(res, "k_a2c_grad")
    assert sorted(single) == OBS_DIMS
    regs = lambda x: x["vgpr_count"] + x["agpr_count"]
    for od in OBS_DIMS:
        print(f"k_apop_grad<{od}> vgpr {pop[od]['vgpr_count']} agpr {pop[od]['agpr_count']}; k_a2c_grad<{od}> vgpr "
              f"{single[od]['vgpr_count']} agpr {single[od]['agpr_count']}")
        assert regs(pop[od]) <= regs(single[od]) + 8, (od, pop[od], single[od])


def test_the_existing_families_keep_their_counts():
    res = _resources()
    for family, count in FAMILIES.items():
        assert len([n for n in res if family in n]) == count, family
