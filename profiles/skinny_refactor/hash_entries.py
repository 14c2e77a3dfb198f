#!/usr/bin/env python3
"""Calls every entry of csrc/skinny.hip with seeded inputs and prints one SHA-256 per output, to compare two builds of the library:

    AST_HIP_LIB=/path/to/libast_hip.so python profiles/skinny_refactor/hash_entries.py > hashes.txt

The entries that add with f32 atomics (ast_bigk_gemm, ast_bign_dgrad and their _wide forms) are not bit-stable in either build:
their lines carry the error against torch float64 instead ("err", to be held under 2e-4), and diffing two listings skips them."""
import ctypes as C
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-style-transfer_amd")]
import torch  # noqa: E402
from ast_amd import _lib  # noqa: E402

DEV = "cuda"
NARROW, WIDE = (1, 16, 17, 33, 64), (65, 79, 130)


def rn(*shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(DEV)


def s():
    return torch.cuda.current_stream().cuda_stream


def sha(label, *tensors):
    torch.cuda.synchronize()
    for j, t in enumerate(tensors):
        print(f"{label} out{j} sha256 {hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()}", flush=True)


def err(label, got, ref):
    torch.cuda.synchronize()
    e = float((got.double().cpu() - ref).abs().max() / ref.abs().max())
    print(f"{label} err {e:.2e} {'ok' if e < 2e-4 else 'FAIL'}", flush=True)


def main():
    L, ck = _lib.lib(), _lib.check
    for sfx, rows in (("", NARROW), ("_wide", WIDE)):
        gemm, gemm_ex, wgrad = (getattr(L, f"ast_{n}") for n in (f"skinny_gemm{sfx}", f"skinny_gemm{sfx}_ex", f"linear_wgrad{sfx}"))
        for M in rows:
            for N, K in ((256, 256), (40, 256), (256, 1024)):
                x, w, b = rn(M, K, seed=1), rn(N, K, seed=2, scale=K ** -0.5), rn(N, seed=3)
                mm = (rn(M, N, seed=4) > 0).float() * 1.25
                ctr = torch.tensor([7], dtype=torch.int64, device=DEV)
                for bias, relu in ((False, False), (True, False), (True, True)):
                    y = torch.zeros(M, N, device=DEV)
                    ck(gemm(x.data_ptr(), w.data_ptr(), b.data_ptr() if bias else None, y.data_ptr(), M, N, K, K, N, int(relu), s()))
                    sha(f"ast_skinny_gemm{sfx} M={M} N={N} K={K} bias={int(bias)} relu={int(relu)}", y)
                y, mask = torch.zeros(M, N, device=DEV), torch.zeros(M, N, device=DEV)
                ck(gemm_ex(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), M, N, K, K, N, 0, mm.data_ptr(), None, 0.0, 0, None, s()))
                sha(f"ast_skinny_gemm{sfx}_ex M={M} N={N} K={K} mul_mask", y)
                ck(gemm_ex(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), M, N, K, K, N, 1, None, mask.data_ptr(), 0.25, 12345,
                           ctr.data_ptr(), s()))
                sha(f"ast_skinny_gemm{sfx}_ex M={M} N={N} K={K} dropout", y, mask)
            for N, K in ((40, 100), (256, 256)):
                dy, x = rn(M, N, seed=5), rn(M, K, seed=6)
                for with_db in (True, False):
                    dW, db = rn(N, K, seed=7), rn(N, seed=8)
                    ck(wgrad(dy.data_ptr(), x.data_ptr(), dW.data_ptr(), db.data_ptr() if with_db else None, M, N, K, N, K, s()))
                    sha(f"ast_linear_wgrad{sfx} M={M} N={N} K={K} db={int(with_db)}", dW, db)
            N, K = 256, 2050
            x, w, b = rn(M, K, seed=9, scale=0.1), rn(N, K, seed=10, scale=0.05), rn(N, seed=11, scale=0.1)
            y = torch.zeros(M, N, device=DEV)
            ck(getattr(L, f"ast_bigk_gemm{sfx}")(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), M, N, K, N, s()))
            err(f"ast_bigk_gemm{sfx} M={M} N={N} K={K}", y, x.double().cpu() @ w.double().cpu().t() + b.double().cpu())
            need = int(getattr(L, f"ast_bigk_gemm{sfx}_det_ws_floats")(M, N, K))
            ws = torch.zeros(need, device=DEV)
            ck(getattr(L, f"ast_bigk_gemm{sfx}_det")(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), M, N, K, ws.data_ptr(), need, s()))
            sha(f"ast_bigk_gemm{sfx}_det M={M} N={N} K={K} ws={need}", y)
            N = 2050
            for K in (256, 100):
                dy, w = rn(M, N, seed=12, scale=0.1), rn(N, K, seed=13, scale=0.05)
                dx = torch.zeros(M, K, device=DEV)
                ck(getattr(L, f"ast_bign_dgrad{sfx}")(dy.data_ptr(), w.data_ptr(), dx.data_ptr(), M, N, K, N, s()))
                err(f"ast_bign_dgrad{sfx} M={M} N={N} K={K}", dx, dy.double().cpu() @ w.double().cpu())
                need = int(getattr(L, f"ast_bign_dgrad{sfx}_det_ws_floats")(M, N, K))
                ws = torch.zeros(need, device=DEV)
                ck(getattr(L, f"ast_bign_dgrad{sfx}_det")(dy.data_ptr(), w.data_ptr(), dx.data_ptr(), M, N, K, N, ws.data_ptr(), need, s()))
                sha(f"ast_bign_dgrad{sfx}_det M={M} N={N} K={K} ws={need}", dx)
    # batched forms: distinct destinations, every second record without db
    for label, shapes in (("three", [(5, 40, 100), (17, 256, 256), (64, 70, 130)]), ("57", [(3, 16, 64)] * 57)):
        for form in ("host", "device"):
            keep, recs = [], []
            for j, (M, N, K) in enumerate(shapes):
                dy, x, dW, db = rn(M, N, seed=20 + 4 * j), rn(M, K, seed=21 + 4 * j), rn(N, K, seed=22 + 4 * j), rn(N, seed=23 + 4 * j)
                keep.append((dy, x, dW, db))
                recs.append(_lib.LinWg(dy=dy.data_ptr(), x=x.data_ptr(), dW=dW.data_ptr(), db=db.data_ptr() if j % 2 == 0 else None, M=M, N=N, K=K,
                                       lddy=N, ldw=K, p0=0, p1=0, p2=0))
            arr = (_lib.LinWg * len(recs))(*recs)
            tiles = max(((K + 63) // 64) * ((N + 63) // 64) for _, N, K in shapes)
            if form == "host":
                ck(L.ast_linear_wgrad_batched_host(C.addressof(arr), len(recs), tiles, s()))
            else:
                table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
                ck(L.ast_linear_wgrad_batched(table.data_ptr(), len(recs), tiles, s()))
            sha(f"ast_linear_wgrad_batched{'_host' if form == 'host' else ''} {label} records", torch.cat([k[2].flatten() for k in keep]),
                torch.cat([k[3] for k in keep]))


if __name__ == "__main__":
    main()
