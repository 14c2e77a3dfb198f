#!/usr/bin/env python3
"""Times the ragged-training entries through the C-ABI against the unmasked entries on the same tensors, same process, with the
method of profiles/masked_attn_training/bench_masked_attn.py: the kernels alternate, 5 warm-up + 30 timed repetitions each, device
events around every call; prints the median and the min..max spread.  The unmasked kernels of this library are the parent's code
(profiles/ragged_decoder_training/kernel_diff.txt: 0 differ), so they stand for the parent here.

- ast_recon_loss_len_grad at B = 8, S = 4, T = 287, F = 513 (target row stride 597) against ast_recon_loss_total with a gradient
  pointer; equal lengths and half lengths (2 of 4 sections per clip).
- ast_bign_dgrad_len (default and deterministic form) and ast_linear_wgrad_len at M = 32 (B = 8, S = 4) and M = 256 (B = 8,
  S = 32), N = 294 462, K = 256 against ast_bign_dgrad[_wide][_det] / ast_linear_wgrad[_wide]; full and half lengths; effective
  GB/s over the 301 MB weight stream (the weight gradient reads and writes it: 603 MB).
Usage: python profiles/ragged_decoder_training/bench_ragged_train.py [out.txt]"""
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-style-transfer_amd")]
import torch  # noqa: E402
from ast_amd import _lib  # noqa: E402

REPS, WARM = 30, 5


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


def fmt(t, nbytes=None):
    m = statistics.median(t)
    return f"{m:8.1f} ({min(t):.1f}..{max(t):.1f})" + (f" {nbytes / m / 1e3:6.0f} GB/s" if nbytes else "")


def main():
    L, ck = _lib.lib(), _lib.check
    dev = "cuda"
    lines = []
    # ---- the loss -------------------------------------------------------------------------------------------------------------
    B, S, T, F, ld = 8, 4, 287, 513, 597
    out = torch.randn(B, S, 2, T, F, device=dev)
    x = torch.randn(B, S, 2, T, ld, device=dev)
    grad = torch.empty_like(out)
    n = B * S * T * F
    c = (2.0 / (2 * n), 0.5 / n, 0.2 / n, 0.3 / (2 * B * (S - 1) * T * F), 0.1 / (2 * B * S * (T - 1) * F))
    inv = (1.0 / (2 * n), 1.0 / n, 1.0 / n, 1.0 / (2 * B * (S - 1) * T * F), 1.0 / (2 * B * S * (T - 1) * F))
    c5, i5, w5 = (ctypes.c_float * 5)(*c), (ctypes.c_float * 5)(*inv), (ctypes.c_float * 5)(2.0, 0.5, 0.2, 0.3, 0.1)
    ws0, res0 = torch.empty(64 * 5, device=dev), torch.empty(11, device=dev)
    need = int(L.ast_recon_loss_len_grad_ws_floats(B, S, T, F))
    ws, res, loss = torch.empty(need, device=dev), torch.empty(B, 11, device=dev), torch.empty(1, device=dev)
    full = torch.full((B,), S, dtype=torch.int32, device=dev)
    half = torch.full((B,), S // 2, dtype=torch.int32, device=dev)
    batch = lambda: ck(L.ast_recon_loss_total(out.data_ptr(), x.data_ptr(), ld, B, S, T, F, c5, i5, ws0.data_ptr(), res0.data_ptr(),
                                              grad.data_ptr(), s()), "ast_recon_loss_total")

    def ragged(nsec):
        return lambda: ck(L.ast_recon_loss_len_grad(out.data_ptr(), x.data_ptr(), ld, B, S, T, F, nsec.data_ptr(), None, w5, ws.data_ptr(), need,
                                                    res.data_ptr(), loss.data_ptr(), grad.data_ptr(), s()), "ast_recon_loss_len_grad")

    a, b, h = alternate([batch, ragged(full), ragged(half)])
    m = statistics.median
    lines += [f"loss, B={B} S={S} T={T} F={F}: us median (min..max)",
              f"  ast_recon_loss_total + grad        {fmt(a)}",
              f"  ast_recon_loss_len_grad, full      {fmt(b)}   x{m(b) / m(a):.2f}",
              f"  ast_recon_loss_len_grad, half      {fmt(h)}   x{m(h) / m(a):.2f}"]
    del out, x, grad
    # ---- the masked linear's backward --------------------------------------------------------------------------------------------
    N, K = 294462, 256
    w = torch.randn(N, K, device=dev) * 0.05
    dW, db = torch.zeros(N, K, device=dev), torch.zeros(N, device=dev)
    wbytes = 4.0 * N * K
    for M, Ssec in ((32, 4), (256, 32)):
        nclips = M // Ssec
        dy, xx, dx = torch.randn(M, N, device=dev), torch.randn(M, K, device=dev), torch.empty(M, K, device=dev)
        full = torch.full((nclips,), Ssec, dtype=torch.int32, device=dev)
        half = torch.full((nclips,), Ssec // 2, dtype=torch.int32, device=dev)
        wide = "_wide" if M > 64 else ""
        dneed = int(L.ast_bign_dgrad_len_det_ws_floats(M, N, K))
        dws = torch.empty(dneed, device=dev)
        un = lambda: ck(getattr(L, "ast_bign_dgrad" + wide)(dy.data_ptr(), w.data_ptr(), dx.data_ptr(), M, N, K, N, s()), "dgrad")
        und = lambda: ck(getattr(L, f"ast_bign_dgrad{wide}_det")(dy.data_ptr(), w.data_ptr(), dx.data_ptr(), M, N, K, N, dws.data_ptr(), dneed, s()), "dgrad_det")
        unw = lambda: ck(getattr(L, "ast_linear_wgrad" + wide)(dy.data_ptr(), xx.data_ptr(), dW.data_ptr(), db.data_ptr(), M, N, K, N, K, s()), "wgrad")

        def dlen(nv):
            return lambda: ck(L.ast_bign_dgrad_len(dy.data_ptr(), w.data_ptr(), dx.data_ptr(), M, N, K, N, Ssec, nv.data_ptr(), s()), "dgrad_len")

        def dlend(nv):
            return lambda: ck(L.ast_bign_dgrad_len_det(dy.data_ptr(), w.data_ptr(), dx.data_ptr(), M, N, K, N, Ssec, nv.data_ptr(), dws.data_ptr(),
                                                       dneed, s()), "dgrad_len_det")

        def wlen(nv):
            return lambda: ck(L.ast_linear_wgrad_len(dy.data_ptr(), xx.data_ptr(), dW.data_ptr(), db.data_ptr(), M, N, K, N, K, Ssec, nv.data_ptr(),
                                                     s()), "wgrad_len")

        lines.append(f"M={M} (S={Ssec}), N={N}, K={K}: us median (min..max), GB/s over the weight stream")
        for title, fns, nb in (("dgrad, atomic      ", [un, dlen(full), dlen(half)], wbytes),
                               ("dgrad, determin.   ", [und, dlend(full), dlend(half)], wbytes),
                               ("wgrad              ", [unw, wlen(full), wlen(half)], 2 * wbytes)):
            a, b, h = alternate(fns)
            lines.append(f"  {title} unmasked {fmt(a, nb)} | masked full {fmt(b, nb)} x{m(b) / m(a):.2f} | masked half {fmt(h, nb)} x{m(h) / m(a):.2f}")
            dW.zero_(); db.zero_()
        del dy, xx, dx, dws
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(text + "\n")


if __name__ == "__main__":
    main()
