#!/usr/bin/env python3
"""Device code of two builds of libast_hip.so, compared per kernel symbol (the evidence for a host-only change).

For every AMDGPU code object of both libraries: the disassembly of each function symbol without addresses and encodings, and
each kernel's metadata note (VGPR / AGPR / SGPR counts, spills, fixed LDS, scratch, kernarg size).  Symbols are matched by name
over all code objects, so a changed instantiation order does not count.  Prints the symbols that differ, appear or disappear
and exits 1 if there are any.  Runs on a CPU machine (llvm-objdump, llvm-readelf).

    python tools/kernel_diff.py OLD.so NEW.so
"""
import os
import re
import subprocess
import sys
import tempfile

from det_isa_audit import LLVM, code_objects

META = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size",
        "private_segment_fixed_size", "kernarg_segment_size", "max_flat_workgroup_size")


def _run(tool, *args):
    return subprocess.run([os.path.join(LLVM, tool), *args], check=True, capture_output=True, text=True).stdout


def symbols(lib):
    """({symbol: [instruction text]}, {kernel: {metadata field: value}}) over every code object of the library"""
    code, meta = {}, {}
    with tempfile.TemporaryDirectory() as td:
        for k, co in enumerate(code_objects(lib)):
            path = os.path.join(td, f"co{k}.o")
            open(path, "wb").write(co)
            body = None
            for line in _run("llvm-objdump", "-d", "--no-show-raw-insn", "--mcpu=gfx950", path).splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m:
                    body = code.setdefault(m.group(1), [])
                elif body is not None and line.strip() == "...":
                    pass        # objdump's mark for zero bytes: alignment padding before the next function, not code
                elif body is not None and line.startswith("\t"):
                    body.append(re.sub(r"\s*//.*$", "", line).strip())          # the comment holds the address
            for block in re.split(r"\n  - (?=\.)", _run("llvm-readelf", "--notes", path)):
                f = dict(re.findall(r"^\s{4}\.(\w+):\s+(\S+)$", block, re.M))
                if "name" in f:
                    meta[f["name"]] = {x: f.get(x) for x in META}
    return code, meta


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    (code_a, meta_a), (code_b, meta_b) = symbols(sys.argv[1]), symbols(sys.argv[2])
    gone, new = sorted(set(code_a) - set(code_b)), sorted(set(code_b) - set(code_a))
    differ = []
    for s in sorted(set(code_a) & set(code_b)):
        why = []
        if code_a[s] != code_b[s]:
            why.append(f"code ({len(code_a[s])} -> {len(code_b[s])} instructions)")
        why += [f"{x} {meta_a[s][x]} -> {meta_b[s][x]}" for x in META if s in meta_a and s in meta_b and meta_a[s][x] != meta_b[s][x]]
        if (s in meta_a) != (s in meta_b):
            why.append("kernel metadata on one side only")
        if why:
            differ.append((s, why))
    print(f"{len(code_a)} -> {len(code_b)} function symbols, {len(meta_a)} -> {len(meta_b)} kernels with metadata, "
          f"{sum(map(len, code_a.values()))} -> {sum(map(len, code_b.values()))} instructions")
    for title, names in (("disappeared", gone), ("appeared", new)):
        for s in names:
            print(f"{title}: {s}")
    for s, why in differ:
        print(f"differs: {s}: {'; '.join(why)}")
    print(f"{len(differ)} differ, {len(new)} appeared, {len(gone)} disappeared")
    return 1 if differ or new or gone else 0


if __name__ == "__main__":
    sys.exit(main())
