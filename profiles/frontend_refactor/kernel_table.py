#!/usr/bin/env python3
"""Per-kernel allocation of the front-end kernels in two builds of libast_hip.so, as a table (every cell parent/new):

    python profiles/frontend_refactor/kernel_table.py PARENT.so NEW.so > kernel_table.txt

VGPR, SGPR, fixed LDS bytes, scratch bytes and spills from the kernels' metadata; instructions, global loads and barriers counted
in the disassembly (tools/kernel_diff.py does both)."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from kernel_diff import symbols  # noqa: E402

NAMES = ("cqt_octave_", "decimate2_", "cqt_sections_", "stft_sections_", "istft_frames_", "istft_ola_", "overlap_avg_")


def main():
    (code_a, meta_a), (code_b, meta_b) = symbols(sys.argv[1]), symbols(sys.argv[2])
    print("kernel | same code | VGPR | SGPR | LDS | scratch | spills | instructions | global loads | barriers")
    for sym in sorted(s for s in meta_a if any(n in s for n in NAMES)):
        m = re.match(r"_ZN12_GLOBAL__N_1\d+([a-z0-9_]+?)(?:ILi(\d+)EE)?E", sym)          # name and template argument of the mangled symbol
        short = m.group(1) + (f"<{m.group(2)}>" if m.group(2) else "")
        a, b = meta_a[sym], meta_b[sym]
        cell = lambda f: f"{f(code_a[sym], a)}/{f(code_b[sym], b)}"
        print(" | ".join([short, "yes" if code_a[sym] == code_b[sym] else "no", cell(lambda c, m: m["vgpr_count"]), cell(lambda c, m: m["sgpr_count"]),
                          cell(lambda c, m: m["group_segment_fixed_size"]), cell(lambda c, m: m["private_segment_fixed_size"]),
                          cell(lambda c, m: int(m["vgpr_spill_count"]) + int(m["sgpr_spill_count"])), cell(lambda c, m: len(c)),
                          cell(lambda c, m: sum(i.startswith("global_load") for i in c)), cell(lambda c, m: sum(i.startswith("s_barrier") for i in c))]))


if __name__ == "__main__":
    main()
