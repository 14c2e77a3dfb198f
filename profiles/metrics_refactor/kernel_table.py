#!/usr/bin/env python3
"""Per-kernel allocation of the kernels of csrc/metrics.hip, chroma.hip and curation.hip whose code differs between two builds of
libast_hip.so, as a table (every cell parent/new):

    python profiles/metrics_refactor/kernel_table.py PARENT.so NEW.so > kernel_table.txt

VGPR, SGPR, fixed LDS bytes, scratch bytes and spills from the kernels' metadata; instructions, global loads and barriers counted
in the disassembly (tools/kernel_diff.py does both).  Waves per SIMD: what the VGPR count allows a 256-thread workgroup's waves on
gfx950 (512 VGPRs per SIMD lane, allocated in steps of 8, at most 8 waves)."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from kernel_diff import symbols  # noqa: E402


def waves(vgpr):
    return min(8, 512 // (-(-int(vgpr) // 8) * 8))


def main():
    (code_a, meta_a), (code_b, meta_b) = symbols(sys.argv[1]), symbols(sys.argv[2])
    names = sorted(s for s in meta_a if s in meta_b and (code_a[s] != code_b[s] or meta_a[s] != meta_b[s]))
    print("kernel | VGPR | waves per SIMD | SGPR | LDS | scratch | spills | instructions | global loads | barriers")
    for sym in names:
        m = re.match(r"_ZN12_GLOBAL__N_1\d+([a-z0-9_]+?)(?:I((?:Lb[01]E)+)E)?E", sym)          # name and bool template arguments of the mangled symbol
        name = m.group(1) + ("<" + ", ".join(re.findall(r"Lb([01])E", m.group(2))) + ">" if m.group(2) else "")
        a, b = meta_a[sym], meta_b[sym]
        cell = lambda f: f"{f(code_a[sym], a)}/{f(code_b[sym], b)}"
        print(" | ".join([name, cell(lambda c, m: m["vgpr_count"]),
                          cell(lambda c, m: waves(m["vgpr_count"])), cell(lambda c, m: m["sgpr_count"]),
                          cell(lambda c, m: m["group_segment_fixed_size"]), cell(lambda c, m: m["private_segment_fixed_size"]),
                          cell(lambda c, m: int(m["vgpr_spill_count"]) + int(m["sgpr_spill_count"])), cell(lambda c, m: len(c)),
                          cell(lambda c, m: sum(i.startswith("global_load") for i in c)), cell(lambda c, m: sum(i.startswith("s_barrier") for i in c))]))


if __name__ == "__main__":
    main()
