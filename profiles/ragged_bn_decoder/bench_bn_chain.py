#!/usr/bin/env python3
"""Times forward + backward of conv_decoder's four convT+BN+ReLU layers of new_decoder.Decoder on N = 32 images (B = 8 clips of
S = 4 sections, input (32, 32, 16, 8) NHWC, output (32, 512, 256, 8)): the unmasked chain (layers.convT_bn_act, training mode,
the configured fusions) against the masked one (layers.convT_bn_act_len) at full lengths and at half lengths (every clip
n_b = S / 2).  Seeded weights, both compute dtypes, eager launches.  The three variants alternate, 10 warm-up rounds and 40 timed
repetitions each, device events around each repetition; prints median, min, 10th / 90th percentile and max in ms.
Usage: python profiles/ragged_bn_decoder/bench_bn_chain.py [out.txt]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-style-transfer_amd")]
import torch  # noqa: E402
import ast_amd  # noqa: E402
from ast_amd import config, layers as L, ops  # noqa: E402
from oracle import seeded_params as sp  # noqa: E402

DEV = "cuda"
B, S = 8, 4
REPS, WARM = 40, 10


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None
    for dtype in (torch.bfloat16, torch.float32):
        config.set_compute_dtype(dtype)
        dec = ast_amd.Decoder()
        dec.load_state_dict(sp.seeded_state_dict(dec.state_dict(), tag="decoder"))
        dec = dec.to(DEV).train()
        dec._prepare()
        g = torch.Generator().manual_seed(1)
        h0 = torch.randn(B * S, 32, 16, 8, generator=g).to(DEV).to(dtype)
        h0[..., 1:] = 0                                              # one real channel, as sequence_to_feature gives
        dy = torch.randn(B * S, 512, 256, 8, generator=g).to(DEV).to(dtype)
        full = torch.full((B,), S, dtype=torch.int32, device=DEV)
        half = torch.full((B,), S // 2, dtype=torch.int32, device=DEV)

        def chain(n):
            ops.stat_arena_reset(DEV)
            h = h0.clone().requires_grad_(True)
            for pw, i in zip(dec._dec[:4], (0, 3, 6, 9)):
                bn = dec.conv_decoder[i + 1]
                h = L.convT_bn_act(h, pw, 3, 2, 1, 1, bn, True) if n is None else L.convT_bn_act_len(h, pw, 3, 2, 1, 1, bn, (n, S))
            h.backward(dy)

        variants = (("unmasked", None), ("masked, full lengths", full), ("masked, half lengths", half))
        for _ in range(WARM):
            for _, n in variants:
                chain(n)
        torch.cuda.synchronize()
        times = {k: [] for k, _ in variants}
        for _ in range(REPS):
            for k, n in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                chain(n)
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1))
        for k, v in times.items():
            v.sort()
            line = (f"{dtype} {k}: median {statistics.median(v):.3f} ms, min {v[0]:.3f}, p10 {v[REPS // 10]:.3f}, "
                    f"p90 {v[REPS - 1 - REPS // 10]:.3f}, max {v[-1]:.3f} ({REPS} runs)")
            print(line)
            if out:
                out.write(line + "\n")
    if out:
        out.close()


if __name__ == "__main__":
    main()
