#!/usr/bin/env python3
"""Times the attention core past 16 tokens (ast_attn_fwd_p / ast_attn_bwd_p -> csrc/attn.hip) through the C-ABI against
torch.nn.functional.scaled_dot_product_attention in f32 on the same inputs, same process.

B = 8, H = 4, dh = 64 at (Lq, Lk) = (32, 64), (64, 128), (256, 512).  Alternating A/B, 5 warm-up + 30 timed repetitions each,
device events around every call (a backward call is the three launches of the long path; torch's is autograd.grad through its
own saved forward); prints the median and the min..max spread.  Usage: python profiles/long_attention/bench_attn.py [out.txt]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-style-transfer_amd")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from ast_amd import _lib  # noqa: E402

B, H, DH, REPS, WARM = 8, 4, 64, 30, 5


def s():
    return torch.cuda.current_stream().cuda_stream


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def ab(a, b):
    for _ in range(WARM):
        a(); b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(REPS):
        ta.append(timed(a)); tb.append(timed(b))
    return ta, tb


def fmt(t):
    return f"{statistics.median(t):8.1f} ({min(t):.1f}..{max(t):.1f})"


def main():
    L, ck = _lib.lib(), _lib.check
    d = H * DH
    lines = ["pass  Lq   Lk    attn.hip us (min..max)      torch SDPA f32 us (min..max)   SDPA/attn.hip"]
    for Lq, Lk in ((32, 64), (64, 128), (256, 512)):
        q = torch.randn(B * Lq, d, device="cuda")
        kv = torch.randn(B * Lk, 2 * d, device="cuda")
        g = torch.randn(B * Lq, d, device="cuda")
        o, probs = torch.empty_like(q), torch.empty(B, H, Lq, Lk, device="cuda")
        dq, dkv = torch.empty_like(q), torch.empty_like(kv)
        kp, vp, dkp, dvp = kv.data_ptr(), kv.data_ptr() + 4 * d, dkv.data_ptr(), dkv.data_ptr() + 4 * d
        fwd = lambda: ck(L.ast_attn_fwd_p(q.data_ptr(), kp, vp, o.data_ptr(), probs.data_ptr(), B, H, Lq, Lk, DH, d, 2 * d, d, 0, None,
                                          0.0, 0, None, s()), "ast_attn_fwd")
        bwd = lambda: ck(L.ast_attn_bwd_p(g.data_ptr(), q.data_ptr(), kp, vp, probs.data_ptr(), dq.data_ptr(), dkp, dvp, B, H, Lq, Lk, DH,
                                          d, 2 * d, d, None, 0.0, 0, None, s()), "ast_attn_bwd")
        Q = q.view(B, Lq, H, DH).transpose(1, 2).contiguous().requires_grad_(True)
        K = kv[:, :d].reshape(B, Lk, H, DH).transpose(1, 2).contiguous().requires_grad_(True)
        V = kv[:, d:].reshape(B, Lk, H, DH).transpose(1, 2).contiguous().requires_grad_(True)
        G = g.view(B, Lq, H, DH).transpose(1, 2).contiguous()
        t_fwd = lambda: F.scaled_dot_product_attention(Q, K, V)
        out = F.scaled_dot_product_attention(Q, K, V)
        t_bwd = lambda: torch.autograd.grad(out, (Q, K, V), G, retain_graph=True)
        fwd()
        err = float((o.view(B, Lq, H, DH).transpose(1, 2) - out).abs().max())
        for name, a, b in (("fwd", fwd, t_fwd), ("bwd", bwd, t_bwd)):
            ta, tb = ab(a, b)
            lines.append(f"{name}  {Lq:4d} {Lk:4d}   {fmt(ta)}   {fmt(tb)}   {statistics.median(tb) / statistics.median(ta):6.2f}")
        lines.append(f"      max |o - sdpa| = {err:.2e}")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(text + "\n")


if __name__ == "__main__":
    main()
