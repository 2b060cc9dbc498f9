"""Resources of the sample-order kernel (k_sample_orders, csrc/b747_ppo_order.hip), read on the CPU from
the shipped gfx950 code object (as tests/test_ppo_gae_resources.py).  Integer only, a key and its partner per lane: no
scratch, no VGPR spills, and few enough registers that the 16 waves of a 1,024-thread workgroup fit one CU (four per
SIMD: at most 128 registers).  Its LDS is dynamic, 8 bytes per key of the padded row count: at the entry point's limit
that request, with whatever the code object declares statically, must fit the CU's 160 KiB."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "b747_rl_ctrl_amd", "libb747.so")
HDR = os.path.join(ROOT, "b747_rl_ctrl_amd", "csrc", "b747_ppo_order.h")
pytestmark = pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"),
                                reason="needs the built library and the ROCm LLVM tools")
CU_LDS = 160 * 1024


def _constant(name):
    with open(HDR) as f:
        m = re.search(r"constexpr \w+ %s = (\d+);" % name, f.read())
    assert m, name
    return int(m.group(1))


def test_the_order_kernel_has_no_scratch_no_spills_and_fits_its_workgroup():
    import kernel_resources
    res = kernel_resources.resources(LIB)
    got = {n: f for n, f in res.items() if "k_sample_orders" in n}
    assert len(got) == 1, sorted(got)
    block = _constant("kOrderMaxBlock")
    assert block == 1024
    for name, f in got.items():
        print(name.split("(")[0], f)
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0, (name, f)
        assert f["vgpr_count"] + (f["agpr_count"] or 0) <= 512 // (block // 64 // 4), (name, f)


def test_the_lds_request_at_the_limit_fits_the_cu():
    import kernel_resources
    res = kernel_resources.resources(LIB)
    (f,) = [f for n, f in res.items() if "k_sample_orders" in n]
    rows = _constant("kOrderMaxRows")
    assert rows == 16384 and rows & (rows - 1) == 0          # the limit is its own padded count
    dynamic = 8 * rows
    print(f"static {f['group_segment_fixed_size']} B + dynamic {dynamic} B of {CU_LDS}")
    assert dynamic == 128 * 1024 and f["group_segment_fixed_size"] + dynamic <= CU_LDS
    # the launcher raises the dynamic limit to exactly that request, and only above the default 64 KiB
    with open(os.path.join(ROOT, "b747_rl_ctrl_amd", "csrc", "b747_ppo_order.hip")) as fh:
        src = fh.read()
    assert "hipFuncAttributeMaxDynamicSharedMemorySize" in src and "kOrderMaxRows * sizeof(uint64_t)" in src


def test_the_older_resource_tests_name_filters_do_not_catch_the_new_kernel():
    import kernel_resources
    res = kernel_resources.resources(LIB)
    count = lambda *keys: sum(any(k in n for k in keys) for n in res)
    assert count("k_ppo_gae<") == 1 and count("k_pop_gae") == 1
    assert count("k_ppo_grad<") == 5 and count("k_pop_grad<") == 5 and count("k_hyp_grad<") == 5
