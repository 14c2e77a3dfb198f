#!/usr/bin/env python3
"""Wall time of one eager (uncaptured) Trainer.step, where host glue shows: the bench configuration (B = 8, S = 2, bf16) with
use_graph off, 3 warm-up steps, then 5 steps timed one by one with a device synchronisation on either side; prints the median and
min..max in ms.  --root CHECKOUT: the checkout whose ast_amd is imported (default: this one)."""
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1]) if "--root" in sys.argv else HERE
sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-style-transfer_amd")]
import torch  # noqa: E402
from ast_amd import config, train  # noqa: E402

config.set_compute_dtype(torch.bfloat16)
tr = train.Trainer(train.TrainConfig(use_graph=False), seed=7)
x, labels = train.synthetic_batch(8, 2, "cuda:0", seed=3)
for _ in range(3):
    tr.step(x, labels)
ts = []
for _ in range(5):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr.step(x, labels)
    torch.cuda.synchronize()
    ts.append((time.perf_counter() - t0) * 1e3)
print(f"eager Trainer.step ms: median {statistics.median(ts):.3f} ({min(ts):.3f}..{max(ts):.3f})", flush=True)
