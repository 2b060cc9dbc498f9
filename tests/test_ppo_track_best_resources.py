"""Resources of the control-test bookkeeping kernel (k_track_best, csrc/b747_ppo_track.hip), read on the CPU
from the shipped gfx950 code object (as tests/test_ppo_sample_orders_resources.py).  Three lanes keep eight float64
running sums each and everybody copies 16 bytes a pass: no scratch, no spills, and few enough registers that the kernel
never limits how many members' workgroups share a CU.  Its LDS is static and what the design says: the member's three
windows at the entry point's limit of 128 entries, 8 bytes each, and the 4-byte verdict."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "b747_rl_ctrl_amd", "libb747.so")
HDR = os.path.join(ROOT, "b747_rl_ctrl_amd", "csrc", "b747_ppo_track.h")
pytestmark = pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"),
                                reason="needs the built library and the ROCm LLVM tools")


def _constant(name):
    with open(HDR) as f:
        m = re.search(r"constexpr \w+ %s = (\d+);" % name, f.read())
    assert m, name
    return int(m.group(1))


def test_the_kernel_has_no_scratch_no_spills_and_the_lds_of_its_design():
    import kernel_resources
    res = kernel_resources.resources(LIB)
    got = {n: f for n, f in res.items() if "k_track_best" in n}
    assert len(got) == 1, sorted(got)
    window, block = _constant("kTrackMaxWindow"), _constant("kTrackBlock")
    assert window == 128 and block == 256 and _constant("kTrackMaxRepeat") == 256
    for name, f in got.items():
        print(name.split("(")[0], f)
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0, (name, f)
        # eight waves per SIMD need at most 64 registers a lane; half of that occupancy is plenty for three busy lanes
        assert f["vgpr_count"] + (f["agpr_count"] or 0) <= 128, (name, f)
        lds = 3 * window * 8 + 4
        assert lds <= f["group_segment_fixed_size"] <= lds + 12, (name, f)        # (rounded up to the allocation unit)


def test_the_older_resource_tests_name_filters_do_not_catch_the_new_kernel():
    import kernel_resources
    res = kernel_resources.resources(LIB)
    count = lambda *keys: sum(any(k in n for k in keys) for n in res)
    assert count("k_sample_orders") == 1 and count("k_ppo_gae<") == 1 and count("k_pop_gae") == 1
    assert count("k_ppo_grad<") == 5 and count("k_pop_grad<") == 5 and count("k_hyp_grad<") == 5
