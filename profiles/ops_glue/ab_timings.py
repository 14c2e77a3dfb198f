#!/usr/bin/env python3
"""Parent and new code in alternation on one GPU, both on this checkout's libast_hip.so (AST_HIP_LIB):

    python profiles/ops_glue/ab_timings.py PARENT_CHECKOUT ROUNDS [bench masked eager ...] > timings.txt

Each round runs, for the parent then for this checkout, a fresh process of each chosen script: bench.py --gpus 1 --steps 20
--warmup 5 (ms_per_step), profiles/masked_attn_training/bench_masked_attn.py (the median of every cell, us) and
profiles/ops_glue/eager_step.py (ms).  Prints every figure, then per row: median (min..max) of each side over the rounds, and
whether the new median is not above the parent's own min..max.  Stops at the first process that fails or runs out of time."""
import json
import os
import re
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PARENT, ROUNDS = os.path.abspath(sys.argv[1]), int(sys.argv[2])
WHICH = sys.argv[3:] or ["bench", "masked", "eager"]
ENV = dict(os.environ, AST_HIP_LIB=os.path.join(HERE, "audio-style-transfer_amd", "ast_amd", "libast_hip.so"))


def run(cmd, limit):
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, env=ENV, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(f"{' '.join(cmd)}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return r.stdout


def bench(root):
    out = run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], 300)
    res = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
    return {"bench.py ms_per_step": res["ms_per_step"]}


def masked(root):
    out = run([sys.executable, os.path.join(root, "profiles", "masked_attn_training", "bench_masked_attn.py")], 120)
    rows = {}
    for l in out.splitlines()[1:]:
        name, Lq, Lk = l.split()[:3]
        for col, v in zip(("unmasked", "masked full", "masked half"), re.findall(r"([\d.]+) \(", l)):
            rows[f"bench_masked_attn.py {name} {Lq}x{Lk} {col} us"] = float(v)
    return rows


def eager(root):
    out = run([sys.executable, os.path.join(HERE, "profiles", "ops_glue", "eager_step.py"), "--root", root], 300)
    return {"eager Trainer.step ms": float(re.search(r"median ([\d.]+)", out).group(1))}


def main():
    data = {}
    for r in range(ROUNDS):
        for side, root in (("parent", PARENT), ("new", HERE)):
            for name in WHICH:
                for row, v in {"bench": bench, "masked": masked, "eager": eager}[name](root).items():
                    data.setdefault(row, {"parent": [], "new": []})[side].append(v)
                    print(f"round {r + 1} {side:6s} {row}: {v:.3f}", flush=True)
    print()
    for row, d in data.items():
        p, n = d["parent"], d["new"]
        inside = statistics.median(n) <= max(p)
        print(f"{row} | parent {statistics.median(p):.3f} ({min(p):.3f}..{max(p):.3f}) | new {statistics.median(n):.3f} "
              f"({min(n):.3f}..{max(n):.3f}) | {'inside' if inside else 'NOT inside'}", flush=True)


if __name__ == "__main__":
    main()
