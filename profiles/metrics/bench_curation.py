#!/usr/bin/env python3
"""Dataset screening on the device against what a user had before it, for the 8 clips of bench_metrics.py ([2, 3, 4, 4, 5, 6, 8, 9]
sections, 99.7 s of audio at 22 050 Hz): (a) the host chain on clips that lie in host memory, as after decoding -- NumPy framing for
the frame RMS, the level and the window levels, torch.stft on the CPU plus a dense mel matrix, dB, clamp, DCT and time-mean per clip
(librosa is not installed; this is its chain restated); (b) for mfcc_mean only, the parent's device route: ast_amd.mfcc plus a masked
time-mean in torch.  The device routes start from clips already on the device; "upload" times the copy that (a) does not need.
bench_metrics.py's protocol: 5 warm-up + 30 timed repetitions, the routes alternating inside every repetition; median and min..max
of the wall time with a device synchronisation at both ends.  Run from the repository root on a GPU:
    python profiles/metrics/bench_curation.py"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "audio-style-transfer_amd"), os.path.dirname(os.path.abspath(__file__))):
    sys.path.insert(0, p)
import ast_amd  # noqa: E402
from ast_amd import curation as Cu  # noqa: E402
from ast_amd import metrics as M  # noqa: E402
from bench_metrics import NS, REPS, SECTIONS, WARM, timed  # noqa: E402
from bench_mfcc import dense_filters  # noqa: E402

HBM_ACHIEVABLE = 6.3e12                                   # bytes/s, float4 copy


def dct_rows(n_mfcc=13):
    k, j = np.arange(n_mfcc)[:, None], np.arange(128)[None, :]
    D = np.cos(np.pi * k * (2 * j + 1) / 256) * np.sqrt(2 / 128)
    D[0] *= np.sqrt(0.5)
    return D.astype(np.float32)


def host_levels(clips):
    """per clip in NumPy: librosa.feature.rms's framing, the silent share, the level, the 100 ms windows"""
    out = []
    for x in clips:
        fr = np.lib.stride_tricks.sliding_window_view(np.pad(x, 1024), 2048)[::512]
        rms = np.sqrt(np.mean(fr * fr, axis=1))
        W = len(x) // 2205
        lv = np.sqrt(np.mean(x[:W * 2205].reshape(W, 2205) ** 2, axis=1))
        with np.errstate(divide="ignore"):
            sound = np.mean(20 * np.log10(lv) > -45.0)
        out.append((float(np.mean(rms < 0.005)), float(np.sqrt(np.mean(x * x))), float(sound)))
    return out


def host_mfcc_mean(clips, W, D, window):
    """per clip on the CPU: torch.stft, dense mel matmul, dB, clamp by the clip's maximum, DCT, time-mean"""
    out = []
    for x in clips:
        S = torch.stft(torch.from_numpy(x), 2048, 512, window=window, center=True, pad_mode="constant", return_complex=True).abs() ** 2
        db = 10 * torch.log10(torch.clamp(W @ S, min=1e-10))
        out.append((D @ torch.maximum(db, db.max() - 80)).mean(dim=1))
    return torch.stack(out)


def parent_mfcc_mean(a, na):
    """ast_amd.mfcc (B, 13, T_max) and a masked time-mean on the device"""
    c = M.mfcc(a, na, n_mfcc=13, hop_length=512)
    T = 1 + na // 512
    mask = torch.arange(c.shape[2], device=a.device)[None, :] < T[:, None]
    return (c * mask[:, None, :]).sum(dim=2) / T[:, None]


def main():
    dev = "cuda"
    gen = torch.Generator().manual_seed(9)
    host = 0.1 * torch.randn(len(NS), max(NS), generator=gen)
    host[3] *= 0.02                                       # one clip below the silence threshold
    clips = [host[b, :n].numpy() for b, n in enumerate(NS)]
    a, na = host.to(dev), torch.tensor(NS, dtype=torch.int32, device=dev)
    W, D, window = torch.from_numpy(dense_filters()), torch.from_numpy(dct_rows()), torch.hann_window(2048)
    print(f"8 clips, sections {SECTIONS}, samples {NS} ({sum(NS) / 22050:.1f} s); {WARM} warm-up + {REPS} timed repetitions, alternating")
    res, ref = Cu.screen(a, na), host_levels(clips)
    print("silence_ratio", [f"{v:.4f}" for v in res["silence_ratio"].tolist()], "host", [f"{r[0]:.4f}" for r in ref])
    print("rms_level    ", [f"{v:.5f}" for v in res["rms_level"].tolist()], "host", [f"{r[1]:.5f}" for r in ref])
    print("sound_ratio  ", [f"{v:.4f}" for v in res["sound_ratio"].tolist()], "host", [f"{r[2]:.4f}" for r in ref])
    hm, pm = host_mfcc_mean(clips, W, D, window), parent_mfcc_mean(a, na).cpu()
    mm = res["mfcc_mean"].cpu()
    print(f"mfcc_mean differs from the host chain by at most {float((mm - hm).abs().max()):.3g} and from the parent's device route by "
          f"{float((mm - pm).abs().max()):.3g} on coefficients up to {float(mm.abs().max()):.1f}")
    times = timed({"screen (new kernels, all of it)": lambda: Cu.screen(a, na),
                   "frame RMS + silence + level pass": lambda: Cu.silence_ratio(a, na),
                   "sound_ratio": lambda: Cu.sound_ratio(a, na),
                   "mfcc_mean (new kernels)": lambda: Cu.mfcc_mean(a, na),
                   "rms_normalize": lambda: Cu.rms_normalize(a, na),
                   "(b) ast_amd.mfcc + masked mean": lambda: parent_mfcc_mean(a, na),
                   "(a) host: NumPy framing, levels": lambda: host_levels(clips),
                   "(a) host: torch.stft + mel/DCT mean": lambda: host_mfcc_mean(clips, W, D, window),
                   "upload of the padded batch": lambda: host.to(dev)})
    # the frame-RMS pass against the memory system: every sample of the clips is read once (the 3 halo blocks per tile hit the cache)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(200):
        Cu.silence_ratio(a, na)
    ev[1].record()
    torch.cuda.synchronize()
    per_call = ev[0].elapsed_time(ev[1]) / 200 * 1e-3
    nbytes = 4 * sum(NS)
    print(f"frame-RMS pass back to back (two launches + allocations per call): {per_call * 1e6:.1f} us per call, {nbytes / 1e6:.2f} MB read -> "
          f"{nbytes / per_call / 1e9:.0f} GB/s; at the achievable HBM rate of {HBM_ACHIEVABLE / 1e12:.1f} TB/s the bytes alone take "
          f"{nbytes / HBM_ACHIEVABLE * 1e6:.2f} us: at this size the call is bound by its launches, not by memory")
    return times


if __name__ == "__main__":
    main()
