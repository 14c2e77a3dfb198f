#!/usr/bin/env python3
"""Times the key-masked training core (ast_attn_fwd_len_p / ast_attn_bwd_len_p) through the C-ABI against the unmasked
ast_attn_fwd_p / ast_attn_bwd_p on the same inputs, same process, with the method of profiles/long_attention/bench_attn.py.
The unmasked kernels of this library are the parent's code (profiles/masked_attn_training/kernel_diff.txt: 0 differ), so they
stand for the parent here.

B = 8, H = 4, dh = 64 at (Lq, Lk) = (32, 64), (64, 128), (256, 512), key_period = Lk, p = 0.1 drawn in the kernels; key_len = Lk
(full) and Lk / 2 (half) for every clip.  The forwards alternate (unmasked, masked full, masked half), so do the unmasked and
the masked full backward; the half-length backward runs on its own forward's probs.  5 warm-up + 30 timed repetitions each,
device events around every call (a backward call is the three launches of the long path); prints the median and the min..max
spread.  Usage: python profiles/masked_attn_training/bench_masked_attn.py [out.txt]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-style-transfer_amd")]
import torch  # noqa: E402
from ast_amd import _lib  # noqa: E402

B, H, DH, REPS, WARM, P, SEED = 8, 4, 64, 30, 5, 0.1, 0x5EED


def s():
    return torch.cuda.current_stream().cuda_stream


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def alternate(fns):
    for _ in range(WARM):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(REPS):
        for t, f in zip(ts, fns):
            t.append(timed(f))
    return ts


def fmt(t):
    return f"{statistics.median(t):8.1f} ({min(t):.1f}..{max(t):.1f})"


def main():
    L, ck = _lib.lib(), _lib.check
    d = H * DH
    lines = ["pass  Lq   Lk    unmasked us (min..max)     masked, full us (min..max)   masked, half us (min..max)   full/unm  half/unm"]
    ctr = torch.zeros(1, dtype=torch.int64, device="cuda")
    for Lq, Lk in ((32, 64), (64, 128), (256, 512)):
        q = torch.randn(B * Lq, d, device="cuda")
        kv = torch.randn(B * Lk, 2 * d, device="cuda")
        g = torch.randn(B * Lq, d, device="cuda")
        o, probs = torch.empty_like(q), torch.empty(B, H, Lq, Lk, device="cuda")
        dq, dkv = torch.empty_like(q), torch.empty_like(kv)
        kp, vp, dkp, dvp = kv.data_ptr(), kv.data_ptr() + 4 * d, dkv.data_ptr(), dkv.data_ptr() + 4 * d
        full = torch.full((B,), Lk, dtype=torch.int32, device="cuda")
        half = torch.full((B,), Lk // 2, dtype=torch.int32, device="cuda")
        fwd = lambda: ck(L.ast_attn_fwd_p(q.data_ptr(), kp, vp, o.data_ptr(), probs.data_ptr(), B, H, Lq, Lk, DH, d, 2 * d, d, 0, None,
                                          P, SEED, ctr.data_ptr(), s()), "ast_attn_fwd_p")
        bwd = lambda: ck(L.ast_attn_bwd_p(g.data_ptr(), q.data_ptr(), kp, vp, probs.data_ptr(), dq.data_ptr(), dkp, dvp, B, H, Lq, Lk, DH,
                                          d, 2 * d, d, None, P, SEED, ctr.data_ptr(), s()), "ast_attn_bwd_p")

        def fwd_len(n):
            return lambda: ck(L.ast_attn_fwd_len_p(q.data_ptr(), kp, vp, o.data_ptr(), probs.data_ptr(), B, H, Lq, Lk, DH, d, 2 * d, d, 0,
                                                   n.data_ptr(), Lk, None, P, SEED, ctr.data_ptr(), s()), "ast_attn_fwd_len_p")

        def bwd_len(n):
            return lambda: ck(L.ast_attn_bwd_len_p(g.data_ptr(), q.data_ptr(), kp, vp, probs.data_ptr(), dq.data_ptr(), dkp, dvp, B, H, Lq,
                                                   Lk, DH, d, 2 * d, d, n.data_ptr(), Lk, None, P, SEED, ctr.data_ptr(), s()),
                              "ast_attn_bwd_len_p")

        tf = alternate([fwd, fwd_len(full), fwd_len(half)])
        fwd_len(half)()                                    # a backward reads the probs of its own forward
        t_half = alternate([bwd_len(half)])[0]
        fwd()                                              # full lengths: the same probs bit for bit, masked or not
        t_un, t_full = alternate([bwd, bwd_len(full)])
        for name, (a, b, c) in (("fwd", tf), ("bwd", (t_un, t_full, t_half))):
            m = statistics.median
            lines.append(f"{name}  {Lq:4d} {Lk:4d}   {fmt(a)}   {fmt(b)}   {fmt(c)}   {m(b) / m(a):6.2f}    {m(c) / m(a):6.2f}")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(text + "\n")


if __name__ == "__main__":
    main()
