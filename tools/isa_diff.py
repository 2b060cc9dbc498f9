"""Per-kernel comparison of two built libraries' gfx950 code: for each kernel whether its instructions are identical,
else the size of the unified diff and the opcode histogram's delta, and the resource counts (VGPR, AGPR, SGPR / VGPR
spills, scratch, LDS) of both.  For refactors that must not change the generated code.
Usage: python tools/isa_diff.py old.so new.so [name-substring ...]   (exit status 1 if the kernel sets differ)"""
import difflib
import os
import re
import subprocess
import sys
from collections import Counter

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_pk_hazard import base_op, kernels   # noqa: E402
from kernel_resources import resources      # noqa: E402

FIELDS = (("vgpr_count", "vgpr"), ("agpr_count", "agpr"), ("sgpr_spill_count", "sspill"), ("vgpr_spill_count", "vspill"),
          ("private_segment_fixed_size", "scratch"), ("group_segment_fixed_size", "lds"))


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return dict(zip(names, out.splitlines()))


def normalise(body):
    """the body with the pc-relative literals masked: the s_add_u32 / s_addc_u32 pair after an s_getpc_b64 holds the
    distance from the instruction to a global (the constant tables), which moves with every kernel laid out in
    between"""
    out, after_pc = [], 0
    for line in body:
        if after_pc and re.match(r"s_addc?_u32 ", line):
            line = re.sub(r", (0x[0-9a-f]+|-?\d+)$", ", <pcrel>", line)
            after_pc -= 1
        else:
            after_pc = 2 if line.startswith("s_getpc_b64") else 0
        out.append(line)
    return out


def load(so):
    bodies = dict(kernels(so))
    dem = demangle(list(bodies))
    return {dem[k]: normalise(v) for k, v in bodies.items()}, resources(so)


def histogram(body):
    return Counter(base_op(line.split()[0]) for line in body)


def main(argv):
    old, new, pats = argv[0], argv[1], argv[2:]
    (bo, ro), (bn, rn) = load(old), load(new)
    print(f"kernels: {len(bo)} old, {len(bn)} new; only old: {sorted(set(bo) - set(bn))}; only new: {sorted(set(bn) - set(bo))}")
    same = 0
    for name in sorted(set(bo) & set(bn)):
        if pats and not any(p in name for p in pats):
            continue
        short = name.replace("(anonymous namespace)::", "").split("(")[0]
        res = " ".join(f"{tag} {ro[name][key]}" + ("" if ro[name][key] == rn[name][key] else f"->{rn[name][key]}")
                       for key, tag in FIELDS)
        if bo[name] == bn[name]:
            same += 1
            print(f"{short}: identical ({len(bn[name])} instructions); {res}")
            continue
        nd = sum(1 for line in difflib.unified_diff(bo[name], bn[name], lineterm="", n=0)
                 if line[:1] in "+-" and line[:3] not in ("+++", "---"))
        ho, hn = histogram(bo[name]), histogram(bn[name])
        delta = {op: hn[op] - ho[op] for op in sorted(set(ho) | set(hn)) if hn[op] != ho[op]}
        print(f"{short}: DIFFERS {len(bo[name])} -> {len(bn[name])} instructions, {nd} diff lines; "
              f"opcode histogram {'unchanged' if not delta else delta}; {res}")
    print(f"identical: {same}")
    return 0 if set(bo) == set(bn) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
