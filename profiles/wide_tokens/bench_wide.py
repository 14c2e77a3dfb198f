#!/usr/bin/env python3
"""Times the wide entries (ast_bigk_gemm_wide, ast_bign_dgrad_wide, ast_linear_wgrad_wide) at the simple decoder's real size
(294 462 x 256) against the <= 64-row entry points called once per 64-row block of the same rows.

Alternating A/B, 5 warm-up + 20 timed repetitions each, device events around every call; prints median and the min..max spread
(the baseline's spread is the noise margin).  Usage: python profiles/wide_tokens/bench_wide.py [out.txt]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-style-transfer_amd")]
import torch  # noqa: E402
from ast_amd import _lib  # noqa: E402

BIG, D, REPS, WARM = 2 * 287 * 513, 256, 20, 5


def s():
    return torch.cuda.current_stream().cuda_stream


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def ab(wide, blocked):
    for _ in range(WARM):
        wide(); blocked()
    torch.cuda.synchronize()
    tw, tb = [], []
    for _ in range(REPS):
        tw.append(timed(wide)); tb.append(timed(blocked))
    return tw, tb


def main():
    L = _lib.lib()
    ck = _lib.check
    w_in = torch.randn(D, BIG, device="cuda") * 0.01        # stft_to_embedding.weight
    w_out = torch.randn(BIG, D, device="cuda") * 0.01       # embedding_to_stft.weight
    b = torch.zeros(D, device="cuda")
    gw_in, gw_out, gb_out = torch.zeros_like(w_in), torch.zeros_like(w_out), torch.zeros(BIG, device="cuda")
    lines = ["op              M  wide us (min..max)        blocked <=64 us (min..max)   blocked/wide"]
    for M in (66, 128, 256):
        x = torch.randn(M, BIG, device="cuda") * 0.1
        h = torch.randn(M, D, device="cuda")
        y, dx = torch.empty(M, D, device="cuda"), torch.empty(M, D, device="cuda")
        blocks = [(m0, min(64, M - m0)) for m0 in range(0, M, 64)]
        cases = {
            "bigk_gemm": (lambda: ck(L.ast_bigk_gemm_wide(x.data_ptr(), w_in.data_ptr(), b.data_ptr(), y.data_ptr(), M, D, BIG, D, s())),
                          lambda: [ck(L.ast_bigk_gemm(x[m0].data_ptr(), w_in.data_ptr(), b.data_ptr(), y[m0].data_ptr(), n, D, BIG, D, s()))
                                   for m0, n in blocks]),
            "bign_dgrad": (lambda: ck(L.ast_bign_dgrad_wide(x.data_ptr(), w_out.data_ptr(), dx.data_ptr(), M, BIG, D, BIG, s())),
                           lambda: [ck(L.ast_bign_dgrad(x[m0].data_ptr(), w_out.data_ptr(), dx[m0].data_ptr(), n, BIG, D, BIG, s()))
                                    for m0, n in blocks]),
            "wgrad N=big": (lambda: ck(L.ast_linear_wgrad_wide(x.data_ptr(), h.data_ptr(), gw_out.data_ptr(), gb_out.data_ptr(), M, BIG, D, BIG, D, s())),
                            lambda: [ck(L.ast_linear_wgrad(x[m0].data_ptr(), h[m0].data_ptr(), gw_out.data_ptr(), gb_out.data_ptr(), n, BIG, D, BIG,
                                                           D, s())) for m0, n in blocks]),
            "wgrad K=big": (lambda: ck(L.ast_linear_wgrad_wide(h.data_ptr(), x.data_ptr(), gw_in.data_ptr(), b.data_ptr(), M, D, BIG, D, BIG, s())),
                            lambda: [ck(L.ast_linear_wgrad(h[m0].data_ptr(), x[m0].data_ptr(), gw_in.data_ptr(), b.data_ptr(), n, D, BIG, D, BIG,
                                                           s())) for m0, n in blocks]),
        }
        for name, (wide, blocked) in cases.items():
            tw, tb = ab(wide, blocked)
            mw, mb = statistics.median(tw), statistics.median(tb)
            lines.append(f"{name:12s} {M:4d}  {mw:9.1f} ({min(tw):.1f}..{max(tw):.1f})   {mb:9.1f} ({min(tb):.1f}..{max(tb):.1f})   {mb / mw:5.2f}")
            print(lines[-1], flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
