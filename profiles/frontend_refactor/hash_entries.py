#!/usr/bin/env python3
"""Calls the 14 front-end entries of csrc/fft.hip and csrc/cqt.hip that come in an equal-clip and a per-clip-length form, on seeded
inputs, and prints one SHA-256 per output, to compare two builds of the library:

    AST_HIP_LIB=/path/to/libast_hip.so python profiles/frontend_refactor/hash_entries.py > hashes.txt

None of these kernels adds with atomics, so two builds that compute the same thing print the same lines.  The shapes are the
smallest that reach every instantiation and every guard; outputs start as zeros, so what a kernel leaves unwritten hashes too."""
import ctypes as C
import hashlib
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-style-transfer_amd")]
import torch  # noqa: E402
from ast_amd import _lib  # noqa: E402

DEV = "cuda"
WIN, STEP = 7, 5                       # ast_ns_min(7) = 768


def rn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def s():
    return torch.cuda.current_stream().cuda_stream


def sha(label, *tensors):
    torch.cuda.synchronize()
    for j, t in enumerate(tensors):
        print(f"{label} out{j} sha256 {hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()}", flush=True)


def halved(n, o):
    return -(-n // (1 << o))


def main():
    L, ck, p = _lib.lib(), _lib.check, _lib.ptr
    # STFT sections and CQT sections: T = 9 frames, sections at 0 and 5; the clips hold 9, 6 and 5 frames
    nsamp, S, clips = 2048, 2, i32([2048, 1500, 1024])
    wave, mean, std = rn(3, nsamp, seed=1), rn(2, 513, seed=2) * 0.1, rn(2, 513, seed=3).abs() + 0.5
    for label, tail in (("ast_stft_sections", ()), ("ast_stft_sections_len", (p(clips),))):
        x = torch.zeros(3, S, 2, WIN, 520, device=DEV)
        ck(getattr(L, label)(p(wave), 3, nsamp, p(mean), p(std), p(x), S, WIN, STEP, 520, *tail, s()))
        sha(label, x)
    cq, cmean, cstd = rn(3, 2, 9, 5, seed=4), rn(2, 5, seed=5) * 0.1, rn(2, 5, seed=6).abs() + 0.5
    for label, tail in (("ast_cqt_sections", ()), ("ast_cqt_sections_len", (p(clips), nsamp))):
        x = torch.zeros(3, S, 2, WIN, 9, device=DEV)
        ck(getattr(L, label)(p(cq), 3, 9, 5, p(cmean), p(cstd), p(x), S, WIN, STEP, 9, 3, *tail, s()))
        sha(label, x)
    # inverse STFT and overlap average: clips of 9, 5 and 2 frames, 2, 1 and 1 sections; F_out = 6 of F_in = 8 (the four-bin tail)
    n_frames, n_sec = i32([9, 5, 2]), i32([2, 1, 1])
    spec = rn(3, 2, 9, 513, seed=7)
    for label, tail in (("ast_istft", ()), ("ast_istft_len", (p(n_frames),))):
        frames, out = torch.zeros(3, 9, 1024, device=DEV), torch.zeros(3, 256 * 8, device=DEV)
        ck(getattr(L, label)(p(spec), 3, 9, p(frames), p(out), *tail, s()))
        sha(label, frames, out)
    sec = rn(3, S, 2, WIN, 8, seed=8)
    for label, tail in (("ast_sections_overlap_avg", ()), ("ast_sections_overlap_avg_len", (p(n_sec), p(n_frames)))):
        out = torch.zeros(3, 2, 9, 6, device=DEV)
        ck(getattr(L, label)(p(sec), p(out), 3, S, WIN, STEP, 8, 6, 9, *tail, s()))
        sha(label, out)
    # CQT octaves: three octaves, T = 9 (the last workgroup holds one frame of eight); nfft = 256 with a 5-filter octave takes the
    # register-held taps, nfft = 64 with 13 filters the generic loop
    for nfft, nfs in ((256, (12, 12, 5)), (64, (13, 13, 13))):
        ys = [rn(3, halved(nsamp, o), seed=10 + o) for o in range(3)]
        los = [sum(nfs[o + 1:]) for o in range(3)]
        ld, rows = sum(nfs), max(nfs)
        w_re, w_im, scale = rn(rows, nfft, seed=13), rn(rows, nfft, seed=14), rn(ld, seed=15)
        I = C.c_int * 3
        args = lambda out: ((C.c_void_p * 3)(*[y.data_ptr() for y in ys]), I(*[y.shape[1] for y in ys]), I(256, 128, 64), I(*los), I(*nfs),
                            I(*[rows - f for f in nfs]), 3, 3, p(w_re), p(w_im), p(scale), nfft, p(out), 9, ld, 0)
        for label, tail in (("ast_cqt_octaves", ()), ("ast_cqt_octaves_len", (p(clips), nsamp, WIN, STEP))):
            out = torch.zeros(3, 2, 9, ld, device=DEV)
            ck(getattr(L, label)(*args(out), *tail, s()))
            sha(f"{label} nfft={nfft}", out)
    # 2:1 FIR: one output per thread (odd tap count) and four (m * B = 256 Ki, the threshold; even tap count), equal clips and
    # clips of their own lengths at halving levels 0 and 2
    for B, m, klen in ((3, 1000, 31), (4, 65536, 30)):
        n = 2 * m
        x, taps = rn(B, n, seed=20), rn(1, klen, seed=21)
        y = torch.zeros(B, m, device=DEV)
        ck(L.ast_resample_poly(p(x), B, n, p(taps), 2, 1, klen, (klen - 1) // 2, p(y), m, math.sqrt(2.0), s()))
        sha(f"ast_resample_poly 2:1 B={B} m={m} klen={klen}", y)
        for o in (0, 2):
            row = n << o                                       # the padded row the level-o signal of n samples comes from
            lens = i32(([row, (row * 5) // 8 + 1, 768, row])[:B])
            y = torch.zeros(B, m, device=DEV)
            ck(L.ast_decimate2_len(p(x), B, n, p(taps), klen, (klen - 1) // 2, p(y), m, math.sqrt(2.0), p(lens), row, WIN, STEP, o, s()))
            sha(f"ast_decimate2_len B={B} m={m} klen={klen} o={o}", y)


if __name__ == "__main__":
    main()
