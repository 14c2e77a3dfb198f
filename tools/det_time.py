#!/usr/bin/env python3
"""Cost of deterministic mode: the bench configuration (BASELINE configs[1]: B = 8 clips of 4 s, S = 2, STFT + CQT front end inside
the step, one captured hipGraph, bf16) timed as bench.py times it -- `--warmup` steps, then `--steps` replays ended by a device
barrier -- in default and in deterministic mode on the same box, alternating, `--runs` fresh Trainers each.

    python tools/det_time.py [--runs 3] [--steps 20] [--warmup 5] [--dtype bf16|f32]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "audio-style-transfer_amd"))

import torch  # noqa: E402

import ast_amd  # noqa: E402
from ast_amd import train  # noqa: E402


def one(det, args, dev):
    tr = train.Trainer(train.TrainConfig(deterministic=det), device=dev)
    waves, x, mean, std, labels = train.synthetic_waveform_batch(8, 4.0, dev, seed=1000)
    tr.set_frontend(waves, mean, std, torch.zeros(2, 84, device=dev), torch.full((2, 84), 0.25, device=dev))
    for _ in range(args.warmup):
        tr.step(x, labels)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        tr.step(x, labels)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / args.steps * 1e3
    del tr
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    args = ap.parse_args()
    ast_amd.set_compute_dtype(torch.bfloat16 if args.dtype == "bf16" else torch.float32)
    dev = "cuda:0"
    res = {False: [], True: []}
    for r in range(args.runs):
        for det in (False, True):
            ms = one(det, args, dev)
            res[det].append(ms)
            print(f"run {r}  {'deterministic' if det else 'default      '}  {ms:7.3f} ms/step", flush=True)
    med = {d: sorted(v)[len(v) // 2] for d, v in res.items()}
    for det in (False, True):
        print(f"{'deterministic' if det else 'default'}: " + " / ".join(f"{m:.2f}" for m in res[det]) + f" ms per step (median {med[det]:.2f})")
    print(f"ratio of medians: {med[True] / med[False]:.3f}")


if __name__ == "__main__":
    main()
