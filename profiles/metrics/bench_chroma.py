#!/usr/bin/env python3
"""chroma_similarity and chroma_distance on the device against the route an evaluation has without them, for the 8 clips of
bench_metrics.py ([2, 3, 4, 4, 5, 6, 8, 9] sections, 99.7 s of audio; the tones of tests/chroma_ref.py's fixture, so that there
are peaks to select from): torch.stft per clip on the device, the power spectrogram copied to the host, and the restated chain of
tests/chroma_ref.py in NumPy there.  bench_metrics.py's protocol: 5 warm-up + 30 timed repetitions, the routes alternating
inside every repetition; median and min..max of the wall time with a device synchronisation at both ends.  The tuning pass
(the median by radix selection + the histogram, one workgroup per clip) is reported on its own from the profiler's kernel times.
Run from the repository root on a GPU:  python profiles/metrics/bench_chroma.py"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "audio-style-transfer_amd"), os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))):
    sys.path.insert(0, p)
import ast_amd  # noqa: E402,F401
from ast_amd import metrics as M  # noqa: E402
import chroma_ref as F  # noqa: E402
from bench_metrics import NS, REPS, SECTIONS, WARM, timed  # noqa: E402


def host_chroma(x, n, n_fft, hop, window):
    """torch.stft on the device, |.|^2 to the host, tuning + filter bank + normalisation there"""
    S = (torch.stft(x[:n], n_fft, hop, window=window, center=True, pad_mode="constant", return_complex=True).abs() ** 2).cpu().numpy()
    raw = F.chroma_filters(n_fft, F.tuning_info(S, n_fft)["tuning"], np.float32) @ S
    mx = np.abs(raw).max(axis=0)
    return raw / np.where(mx < F.F32_TINY, 1, mx)


def host_similarity(g, a, ng, na, window):
    out = []
    for b in range(g.shape[0]):
        cg, co = host_chroma(g[b], ng[b], 1024, 256, window), host_chroma(a[b], na[b], 1024, 256, window)
        T = min(cg.shape[1], co.shape[1])
        r = [F.pearson(cg[c, :T], co[c, :T]) for c in range(12)]
        r = [v for v in r if np.isfinite(v)]
        out.append(float(np.mean(r)) if r else 0.0)
    return out


def host_distance(a, g, na, ng, window):
    out = []
    for b in range(a.shape[0]):
        L = min(na[b], ng[b])
        co, cg = host_chroma(a[b], L, 2048, 512, window), host_chroma(g[b], L, 2048, 512, window)
        out.append(float(np.sqrt(((co - cg) ** 2).sum(axis=0)).mean()))
    return out


def kernel_times(fn, reps=10):
    """device time per kernel name of `reps` calls, in microseconds per call, from the profiler"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    out = {}
    for e in prof.key_averages():
        t = getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0)
        if t:
            out[e.key] = t / reps
    return out


def main():
    dev = "cuda"
    n_max = max(NS)
    a = torch.from_numpy(np.stack([F.tones(F.TONES[b % 4], 300 + b, n=n_max) for b in range(len(NS))])).to(dev)
    g = torch.from_numpy(np.stack([0.8 * F.tones(F.TONES[b % 4], 400 + b, n=n_max) for b in range(len(NS))])).to(dev)
    ng_host = [n - 256 * (i % 3) for i, n in enumerate(NS)]
    na, ng = (torch.tensor(v, dtype=torch.int32, device=dev) for v in (NS, ng_host))
    w1, w2 = torch.hann_window(1024, device=dev), torch.hann_window(2048, device=dev)
    print(f"8 clips, sections {SECTIONS}, samples {NS}; {WARM} warm-up + {REPS} timed repetitions, alternating")
    sim, dist = M.chroma_similarity(g, a, ng, na).cpu(), M.chroma_distance(a, g, na, ng).cpu()
    sim_h, dist_h = host_similarity(g, a, ng_host, NS, w1), host_distance(a, g, NS, ng_host, w2)
    print(f"chroma_similarity {sim.tolist()}\n  differs from the host route by at most {float((sim - torch.tensor(sim_h)).abs().max()):.3g}")
    print(f"chroma_distance {dist.tolist()}\n  differs from the host route by at most {float((dist - torch.tensor(dist_h)).abs().max()):.3g}")
    timed({"chroma_similarity (new kernels)": lambda: M.chroma_similarity(g, a, ng, na),
           "chroma_similarity: torch.stft per clip + host chain": lambda: host_similarity(g, a, ng_host, NS, w1),
           "chroma_distance (new kernels)": lambda: M.chroma_distance(a, g, na, ng),
           "chroma_distance: torch.stft per clip + host chain": lambda: host_distance(a, g, NS, ng_host, w2),
           "estimate_tuning alone, one batch (1024, 256)": lambda: M.estimate_tuning(a, na, 1024, 256),
           "chroma_stft with the tuning supplied, one batch (1024, 256)": lambda: M.chroma_stft(a, na, 1024, 256, tuning=torch.zeros(len(NS), device=dev)),
           "pitch_correlation (new kernels)": lambda: M.pitch_correlation(a, g, na, ng)})
    try:
        for name, fn in (("chroma_similarity", lambda: M.chroma_similarity(g, a, ng, na)), ("chroma_distance", lambda: M.chroma_distance(a, g, na, ng))):
            kt = kernel_times(fn)
            print(f"{name}: device time per call by kernel (profiler), microseconds")
            for k, t in sorted(kt.items(), key=lambda kv: -kv[1]):
                print(f"  {t:10.1f}  {k[:110]}")
    except Exception as e:                                             # the profiler is optional; the wall times above stand
        print(f"kernel times not measured: {type(e).__name__}: {e}")


if __name__ == "__main__":
    main()
