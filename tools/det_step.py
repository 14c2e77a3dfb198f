#!/usr/bin/env python3
"""Deterministic train steps for the kernel list of tools/det_isa_audit.py: the bench configuration (B = 8, S = 2, STFT + CQT front
end, one captured graph) in bf16 and f32, and decoder="simple" in f32 (B = 2, S = 1), two steps each.  Run it under
`rocprofv3 --kernel-trace --stats -d DIR -o det -- python tools/det_step.py`; the kernel-stats CSV is the list (profiles/r04/)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "audio-style-transfer_amd"))

import torch  # noqa: E402

import ast_amd  # noqa: E402
from ast_amd import train  # noqa: E402

dev = "cuda:0"
with ast_amd.deterministic():
    for dt in (torch.bfloat16, torch.float32):
        ast_amd.set_compute_dtype(dt)
        tr = train.Trainer(train.TrainConfig(dropout=False), device=dev)
        waves, x, mean, std, labels = train.synthetic_waveform_batch(8, 4.0, dev, seed=1000)
        tr.set_frontend(waves, mean, std, torch.zeros(2, 84, device=dev), torch.full((2, 84), 0.25, device=dev))
        for _ in range(2):
            tr.step(x, labels)
        torch.cuda.synchronize()
    ast_amd.set_compute_dtype(torch.float32)
    tr = train.Trainer(train.TrainConfig(dropout=False, decoder="simple"), device=dev)
    x, labels = train.synthetic_batch(2, 1, dev, seed=3)
    for _ in range(2):
        tr.step(x, labels)
    torch.cuda.synchronize()
print("deterministic steps done")
