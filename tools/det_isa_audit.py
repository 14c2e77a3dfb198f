#!/usr/bin/env python3
"""Float atomics in the gfx950 code objects of libast_hip.so, per kernel symbol (deterministic mode).

Disassembles every AMDGPU code object embedded in the library's .hip_fatbin section and counts, per kernel, the float-adding
atomic instructions (global_ / buffer_ / flat_atomic_add_f32 / _f64 / _pk_add_*).  With --kernels LIST (one kernel name per line,
or the kernel-stats CSV of a `rocprofv3 --kernel-trace --stats` run of a deterministic step: profiles/r04/) it checks every
listed kernel that lives in the library and exits 1 if any of them holds one; kernels not in the library (ATen's) are listed
apart.  Without --kernels it prints every kernel that holds float atomics.  Runs on a CPU machine (llvm-objdump).

    python tools/det_isa_audit.py [--lib PATH] [--kernels profiles/r04/det_step_kernels.txt]
"""
import argparse
import collections
import csv
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
FLOAT_ATOMIC = re.compile(r"^\s*(global|buffer|flat)_atomic_(add_f32|add_f64|pk_add_\w+)\b")


def code_objects(lib):
    """The AMDGPU ELF images inside the library's .hip_fatbin section."""
    with tempfile.TemporaryDirectory() as td:
        fb = os.path.join(td, "fatbin")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fb}", lib, os.path.join(td, "lib.copy")], check=True)
        data = open(fb, "rb").read()
    out, i = [], data.find(b"\x7fELF")
    while i >= 0:
        e_machine = struct.unpack_from("<H", data, i + 18)[0]
        e_shoff, = struct.unpack_from("<Q", data, i + 40)
        e_shentsize, e_shnum = struct.unpack_from("<HH", data, i + 58)
        end = i + e_shoff + e_shentsize * e_shnum
        if e_machine == 0xE0:                         # EM_AMDGPU
            out.append(data[i:end])
        i = data.find(b"\x7fELF", max(end, i + 4))
    return out


def _disassemble(path, demangled):
    """[(kernel label, float atomics)] in file order"""
    cmd = [os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--mcpu=gfx950", path] + (["-C"] if demangled else [])
    out = []
    for line in subprocess.run(cmd, check=True, capture_output=True, text=True).stdout.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            out.append([m.group(1), 0])
        elif out and FLOAT_ATOMIC.match(line):
            out[-1][1] += 1
    return out


def atomics_per_kernel(lib):
    """{name: float atomics}, every kernel under its mangled name and its normalised demangled name (the profiler reports
    the demangled form, or the mangled one where its demangler gives up, e.g. on __bf16 template arguments)"""
    counts = collections.Counter()
    with tempfile.TemporaryDirectory() as td:
        for k, co in enumerate(code_objects(lib)):
            path = os.path.join(td, f"co{k}.o")
            open(path, "wb").write(co)
            for (mangled, c), (dem, _) in zip(_disassemble(path, False), _disassemble(path, True)):
                counts[mangled] += c
                counts[norm(dem)] += c
    return counts


def norm(name):
    """Kernel name without return type, argument list, clone suffix or spaces: 'ns::kernel<args>'."""
    s = name.strip()
    if s.startswith("void "):
        s = s[5:]
    s = re.sub(r"\.kd$", "", s)
    if s.endswith(")"):                               # drop the trailing parameter list (the name itself may hold parentheses)
        depth = 0
        for j in range(len(s) - 1, -1, -1):
            depth += s[j] == ")"
            depth -= s[j] == "("
            if depth == 0:
                s = s[:j]
                break
    return re.sub(r"\s+", "", s)


def read_list(path):
    if path.endswith(".csv"):
        with open(path, newline="") as f:
            rows = list(csv.DictReader(f))
        col = next(c for c in ("Name", "KERNEL_NAME", "Kernel_Name", "kernel_name") if rows and c in rows[0])
        return [r[col] for r in rows]
    return [l.rstrip("\n") for l in open(path) if l.strip() and not l.startswith("#")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "audio-style-transfer_amd", "ast_amd", "libast_hip.so"))
    ap.add_argument("--kernels", help="kernel names (one per line) or a rocprofv3 kernel-stats CSV")
    args = ap.parse_args()
    by_norm = atomics_per_kernel(args.lib)
    if not args.kernels:
        bad = sorted((n, c) for n, c in by_norm.items() if c and not n.startswith("_Z"))
        print(f"{sum(not n.startswith('_Z') for n in by_norm)} kernels, {len(bad)} with float atomics")
        for n, c in bad:
            print(f"{c:6d}  {n}")
        return 0
    listed = sorted(set(read_list(args.kernels)))
    fails, foreign = 0, []
    for name in listed:
        n = name.strip() if name.strip().startswith("_Z") else norm(name)
        if n not in by_norm:
            # a name the profiler's demangler garbled (bf16 template arguments): every library instantiation of that kernel with
            # the same last template argument (the DET / SLAB selector) is a candidate, and the worst one counts
            base, last = n.split("<")[0], n.rsplit(",", 1)[-1]
            cands = [m for m in by_norm if "<" in n and not m.startswith("_Z") and m.split("<")[0] == base and m.rsplit(",", 1)[-1] == last]
            if not cands:
                foreign.append(n)
                continue
            by_norm[n] = max(by_norm[m] for m in cands)
            n += f"   [resolved over {len(cands)} instantiations]"
        c = by_norm[n.split("   [")[0]]
        fails += c > 0
        print(f"{c:6d}  {n}")
    print(f"{len(listed) - len(foreign)} listed kernels in the library, {fails} with float atomics")
    if foreign:
        print(f"{len(foreign)} listed kernels not in the library (ATen / runtime):")
        for n in foreign:
            print(f"        {n}")
    return 1 if fails else 0


if __name__ == "__main__":
    sys.exit(main())
