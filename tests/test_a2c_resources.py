"""Register and LDS use of the A2C update's kernels, read on the CPU from the shipped gfx950 code object (as
tests/test_ppo_update_resources.py).  k_a2c_grad<obs_dim> is k_ppo_grad<obs_dim>'s body with a row that does strictly
less (no ratio, no clip, no old_logp): it must fit one wave per SIMD with no scratch and no spills, inside the LDS
layout the two share, and in no more VGPRs than its PPO sibling of the same build -- a condition, not a measurement."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "b747_rl_ctrl_amd", "libb747.so")
pytestmark = pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"),
                                reason="needs the built library and the ROCm LLVM tools")
OBS_DIMS = (3, 5, 7, 8, 10)
PH = 64


def _upd_lds_bytes(od):
    """UpdLds<OD>::bytes (csrc/b747_ppo_update.h), the dynamic LDS of the gradient kernels"""
    t2 = 2 * 2 * 32 * 64
    sm = 2 * t2
    net = PH * od + 3 * PH
    ls = sm + 2 * net + 2
    wave = (ls + 1 + 3) & ~3
    per_wave = 2 * PH * 33 + 32 * od + 32
    return (wave + 4 * per_wave) * 4


def _by_obs_dim(res, kernel):
    out = {}
    for name, f in res.items():
        m = re.search(kernel + r"<(\d+)>", name)
        if m:
            assert int(m.group(1)) not in out, name
            out[int(m.group(1))] = f
    return out


def test_the_a2c_kernels_exist_once_each():
    import kernel_resources
    res = kernel_resources.resources(LIB)
    assert sorted(_by_obs_dim(res, "k_a2c_grad")) == list(OBS_DIMS)
    for k in ("k_ppo_rmsprop", "k_a2c_adv_stats", "k_a2c_reduce"):
        assert len([n for n in res if k in n]) == 1, k


def test_no_scratch_no_spills_and_lds_within_the_shared_layout():
    import kernel_resources
    res = kernel_resources.resources(LIB)
    grad = _by_obs_dim(res, "k_a2c_grad")
    small = {n: f for n, f in res.items() if any(k in n for k in ("k_ppo_rmsprop", "k_a2c_adv_stats", "k_a2c_reduce"))}
    for name, f in {**{f"k_a2c_grad<{od}>": f for od, f in grad.items()}, **small}.items():
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0, (name, f)
        assert (f["sgpr_spill_count"] or 0) == 0, (name, f)
    for od, f in grad.items():
        # the metadata holds the static LDS (the advantage statistics and the waves' fp64 sums); the launch adds the
        # dynamic UpdLds<OD>::bytes: the static part within it, the two together inside a CU's 160 KiB
        assert f["group_segment_fixed_size"] <= _upd_lds_bytes(od), (od, f)
        assert f["group_segment_fixed_size"] + _upd_lds_bytes(od) <= 160 * 1024, (od, f)
        assert f["vgpr_count"] <= 512, (od, f)


def test_the_a2c_row_needs_no_more_vgprs_than_the_ppo_row():
    import kernel_resources
    res = kernel_resources.resources(LIB)
    a2c, ppo = _by_obs_dim(res, "k_a2c_grad"), _by_obs_dim(res, "k_ppo_grad")
    assert sorted(ppo) == list(OBS_DIMS)
    for od in OBS_DIMS:
        print(f"obs_dim {od}: k_a2c_grad {a2c[od]['vgpr_count']} VGPRs, k_ppo_grad {ppo[od]['vgpr_count']}")
        assert a2c[od]["vgpr_count"] <= ppo[od]["vgpr_count"], (od, a2c[od], ppo[od])
