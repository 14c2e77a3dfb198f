#!/usr/bin/env python3
"""Times StyleTransferSession on 8 clips of mixed length, section counts [2, 3, 4, 4, 5, 6, 8, 9], bf16, graph replays:

  A  ragged     one replay of the (B = 8, S_max = 9) graph with n_sections on the device
  B1 bucketed   one graph per distinct section count, the clips of that count batched (7 replays: B = 2 at S = 4, else B = 1)
  B2 one-by-one eight B = 1 replays (one more graph: B = 1 at S = 4)

B1 and B2 are what the session offered before n_sections.  Every candidate includes the copies of its inputs into the
graphs' static buffers (what a caller pays).  Alternating A / B1 / B2, 5 warm-up + 30 timed repetitions each, host wall clock
around a synchronised call sequence; prints the median and the min..max spread in ms.
Usage: python profiles/ragged_infer/bench_ragged.py [out.txt]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-style-transfer_amd")]
import torch  # noqa: E402
import ast_amd  # noqa: E402
from ast_amd import config  # noqa: E402
from ast_amd import utilityFunctions as U  # noqa: E402
from ast_amd.infer import StyleTransferSession  # noqa: E402
from oracle import seeded_params as sp  # noqa: E402

N_SEC, REPS, WARM, DEV = [2, 3, 4, 4, 5, 6, 8, 9], 30, 5, "cuda"


def model(tag, ctor):
    m = ctor()
    m.load_state_dict(sp.seeded_state_dict(m.state_dict(), tag=tag))
    return m.to(DEV).eval()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    config.set_compute_dtype(torch.bfloat16)
    sess = StyleTransferSession(model("content", ast_amd.ContentEncoder), model("decoder", ast_amd.Decoder), use_graph=True)
    clips = [sp.seeded_input(1, n, seed=9000 + b)[0].to(DEV) for b, n in enumerate(N_SEC)]
    cls = sp.seeded_normal((len(clips), 256), 9100).to(DEV)
    padded, n_sections = U.pad_sections(clips)
    buckets = {}
    for b, n in enumerate(N_SEC):
        buckets.setdefault(n, []).append(b)
    bucketed = [(torch.stack([clips[b] for b in idx]), cls[idx].contiguous()) for idx in buckets.values()]
    single = [(c[None].contiguous(), cls[b:b + 1].contiguous()) for b, c in enumerate(clips)]
    cands = {
        "A  ragged, one replay at S_max = 9": lambda: sess(padded, cls, n_sections=n_sections),
        f"B1 bucketed, {len(bucketed)} replays": lambda: [sess(x, c) for x, c in bucketed],
        "B2 one by one, 8 replays": lambda: [sess(x, c) for x, c in single],
    }
    for _ in range(WARM):
        for fn in cands.values():
            fn()
    times = {k: [] for k in cands}
    for _ in range(REPS):
        for k, fn in cands.items():
            times[k].append(timed(fn))
    audio_s = sum(256 * (191 * (n - 1) + 287 - 1) for n in N_SEC) / 22050.0
    lines = [f"StyleTransferSession, bf16, 8 clips with section counts {N_SEC} ({audio_s:.1f} s of audio), {torch.cuda.get_device_name(0)}",
             f"graphs held by the session: {len(sess._graphs)}; {WARM} warm-up + {REPS} timed repetitions, alternating; ms per batch of 8 clips"]
    for k, t in times.items():
        lines.append(f"{k:38s} median {statistics.median(t):7.3f}  min {min(t):7.3f}  max {max(t):7.3f}")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(text + "\n")


if __name__ == "__main__":
    main()
