#!/usr/bin/env python3
"""Resources of every kernel of two `hipcc -S --cuda-device-only` listings of csrc/skinny.hip, side by side.

    python profiles/skinny_refactor/isa_table.py PARENT.s NEW.s

Per kernel: VGPRs, AGPRs, SGPRs, LDS bytes, scratch bytes, waves/SIMD (the listing's "Occupancy"), instructions, MFMAs, global loads.
The parent's kernels are listed under the name of the instantiation that replaced them (PARENT_NAMES).  Exits 1 if a kernel
of the <= 64-row entries (RT = 1, linear_wgrad_kernel, the batched kernels) differs in registers, LDS, scratch, MFMAs or loads,
or if a 64-row kernel has scratch or fewer waves/SIMD than the parent's."""
import re
import sys

PARENT_NAMES = (                                           # parent kernel -> the instantiation that replaces it
    (r"skinny_gemm_kernel<(\d+), (\d+)>", r"skinny_gemm_kernel<1, \1, \2>"),
    (r"skinny_gemm_wide_kernel<(\d+), (\d+)>", r"skinny_gemm_kernel<4, \1, \2>"),
    (r"(bigk_gemm|bign_dgrad)_kernel<(\w+)>", r"\1_kernel<1, \2>"),
    (r"(bigk_gemm|bign_dgrad)_wide_kernel<(\w+)>", r"\1_kernel<4, \2>"),
    (r"linear_wgrad_wide_kernel", "linear_wgrad_rows_kernel"),
)
FIELDS = ("vgpr", "agpr", "sgpr", "lds", "scratch", "waves", "insts", "mfma", "loads")


def kernels(path, parent):
    text = open(path).read()
    out = {}
    starts = list(re.finditer(r"^(_Z\w+):", text, re.M))
    for n, m in enumerate(starts):
        sym, body = m.group(1), text[m.end():starts[n + 1].start() if n + 1 < len(starts) else len(text)]
        base, _, targs = re.match(r"_ZN12_GLOBAL__N_1\d+([a-z_0-9]+?_kernel)(I((?:L[ib]\d+E)+)E)?", sym).groups()
        name = base + ("<%s>" % ", ".join(re.findall(r"L[ib](\d+)E", targs)) if targs else "")     # bools print as 0 / 1
        if parent:
            for pat, rep in PARENT_NAMES:
                name = re.sub("^" + pat + "$", rep, name)
        ops = [l.split()[0] for l in body.split("\n") if l.startswith("\t") and not l.strip().startswith((".", ";"))]
        get = lambda key: int(re.search(r"; %s: (\d+)" % key, body).group(1))
        out[name] = dict(vgpr=get("NumVgprs"), agpr=get("NumAgprs"), sgpr=get("TotalNumSgprs"), lds=get("LDSByteSize"), scratch=get("ScratchSize"),
                         waves=get("Occupancy"), insts=len(ops), mfma=sum(o.startswith("v_mfma") for o in ops),
                         loads=sum(o.startswith(("global_load", "buffer_load", "flat_load")) for o in ops))
    return out


def main():
    old, new = kernels(sys.argv[1], True), kernels(sys.argv[2], False)
    bad = 0
    print("%-46s %s" % ("kernel (parent / new)", " ".join("%9s" % f for f in FIELDS)))
    for name in sorted(set(old) | set(new)):
        a, b = old.get(name), new.get(name)
        if a is None or b is None:
            print("%-46s only in the %s listing" % (name, "new" if a is None else "parent"))
            bad += 1
            continue
        narrow = "_kernel<4, " not in name and "rows_kernel" not in name
        keys = ("vgpr", "agpr", "sgpr", "lds", "scratch", "mfma", "loads") if narrow else ()
        wrong = [f for f in keys if a[f] != b[f]] + (["scratch"] if b["scratch"] else []) + (["waves"] if b["waves"] < a["waves"] else [])
        print("%-46s %s%s" % (name, " ".join("%9s" % ("%d/%d" % (a[f], b[f])) for f in FIELDS), "   <-- " + ",".join(wrong) if wrong else ""))
        bad += bool(wrong)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
