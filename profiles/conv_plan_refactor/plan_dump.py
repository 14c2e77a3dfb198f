"""Every answer of the four conv-plan query functions (ast_igemm_plan, ast_pconv_variant, ast_igemm_ws_floats,
ast_igemm_ws_floats_det) over a grid of geometries, dtypes and planner environments.  CPU only, no launch.  Run once per library in
a process of its own (the knobs that are read once stay at their defaults):

    AST_HIP_LIB=<parent or new libast_hip.so> python profiles/conv_plan_refactor/plan_dump.py [--lines FILE] > plans_<build>.txt

The output is one "environment  number of lines  SHA-256 of the lines" row per environment (the lines themselves run to hundreds of
megabytes); --lines writes the lines of the first environment as well.  `diff` of the two builds' outputs must be empty."""
import ctypes
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "audio-style-transfer_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

from ast_amd import _lib, ops  # noqa: E402
import igemm_cases  # noqa: E402

NS, HWS, CHANS = (1, 2, 16), ((5, 10), (9, 19), (18, 38), (36, 75), (72, 150), (144, 299)), (8, 16, 24, 32, 64, 128, 256, 512)
PLANNER_VARS = igemm_cases.case_env.VARS


def geometries():
    """(label, Gather): every geometry builder of ops.py -- conv forward, its data gradient (all stride-2 parity classes), transposed
    conv forward (all classes) and linear."""
    for N in NS:
        for H, W in HWS:
            for Cs in CHANS:
                for Cd in CHANS:
                    for k in (1, 3):
                        for s in (1, 2):
                            pad = k // 2
                            tag = f"N{N} {H}x{W} {Cs}->{Cd} k{k} s{s}"
                            g, (Ho, Wo) = ops.gather_direct(N, H, W, Cs, Cd, k, s, pad)
                            yield f"fwd {tag}", g
                            for i, gt in enumerate(ops.gathers_transposed(N, Ho, Wo, Cd, H, W, Cs, k, s, pad)):
                                yield f"dgrad{i} {tag}", gt
                            op = s - 1 if k == 3 else 0
                            Ht, Wt = (H - 1) * s - 2 * pad + k + op, (W - 1) * s - 2 * pad + k + op
                            for i, gt in enumerate(ops.gathers_transposed(N, H, W, Cs, Ht, Wt, Cd, k, s, pad)):
                                yield f"convT{i} {tag}", gt
        for rows in (N, 17 * N, 274 * N):
            for Cs in CHANS:
                for Cd in CHANS:
                    yield f"linear rows{rows} {Cs}->{Cd}", ops.gather_direct(rows, 1, 1, Cs, Cd, 1, 1, 0)[0]


def environments():
    envs = [{}, {"AST_PCONV": "0"}] + [{"AST_PCONV_WALL": str(v)} for v in (0, 1, 2)] + [{"AST_PCONV_NF": str(v)} for v in (8, 12, 16)]
    envs.append({"AST_PCONV_MIN_TILES": "1"})
    forces = sorted({dict(c.env)["AST_IGEMM_FORCE"] for c in igemm_cases.CASES if "AST_IGEMM_FORCE" in dict(c.env)})
    return envs + [{"AST_IGEMM_FORCE": f} for f in forces]


def main():
    lines_path = sys.argv[sys.argv.index("--lines") + 1] if "--lines" in sys.argv else None
    lib = _lib.lib()
    geoms = list(geometries())
    out5, out4 = (ctypes.c_int32 * 5)(), (ctypes.c_int32 * 4)()
    for n, env in enumerate(environments()):
        for v in PLANNER_VARS:
            os.environ.pop(v, None)
        os.environ.update(env)
        name = ",".join(f"{k}={v}" for k, v in env.items()) or "(empty)"
        h, count = hashlib.sha256(), 0
        keep = open(lines_path, "w") if lines_path and n == 0 else None
        for label, g in geoms:
            for dt in (_lib.F32, _lib.BF16):
                for i in range(5):
                    out5[i] = -777
                for i in range(4):
                    out4[i] = -777
                rp = lib.ast_igemm_plan(g, dt, ctypes.byref(out5))
                rv = lib.ast_pconv_variant(g, dt, ctypes.byref(out4))
                line = (f"{label} dt{dt} plan {rp} {list(out5)} variant {rv} {list(out4)} ws {lib.ast_igemm_ws_floats(g, dt)} "
                        f"ws_det {lib.ast_igemm_ws_floats_det(g, dt)}\n")
                h.update(line.encode())
                count += 1
                if keep:
                    keep.write(line)
        if keep:
            keep.close()
        print(f"{name}  {count}  {h.hexdigest()}", flush=True)


if __name__ == "__main__":
    main()
