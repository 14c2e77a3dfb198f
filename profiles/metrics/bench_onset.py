#!/usr/bin/env python3
"""onset_accuracy and self_similarity_distance on the device against what an evaluation had before them, for the 8 clips of
bench_metrics.py ([2, 3, 4, 4, 5, 6, 8, 9] sections, 99.7 s of audio): onsets, torch.stft on the device plus the restated chain
(mel, dB, envelope, peak picking, F1) on the host per clip; self-similarity, ast_amd.mfcc on the device plus a copy to the host and
sklearn's NearestNeighbors per clip.  bench_metrics.py's protocol: 5 warm-up + 30 timed repetitions, the routes alternating inside
every repetition; median and min..max of the wall time with a device synchronisation at both ends.  Run from the repository root
on a GPU:  python profiles/metrics/bench_onset.py [--session]
--session also times one transfer_and_score replay with and without onsets=True, self_similarity=True (seeded models)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "audio-style-transfer_amd"), os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))):
    sys.path.insert(0, p)
import ast_amd  # noqa: E402
from ast_amd import metrics as M  # noqa: E402
from bench_metrics import NS, REPS, SECTIONS, WARM, timed  # noqa: E402
from bench_mfcc import dense_filters  # noqa: E402
import onset_ref as F  # noqa: E402


def onsets_host_route(a, g, na, ng, W, window):
    """torch.stft on the device, the power spectrogram copied to the host, then the chain of tests/onset_ref.py per clip"""
    out = []
    for b in range(a.shape[0]):
        L = min(na[b], ng[b])
        masks = []
        for x in (a, g):
            S = (torch.stft(x[b, :L], 2048, 512, window=window, center=True, pad_mode="constant", return_complex=True).abs() ** 2).cpu().numpy()
            db = 10 * np.log10(np.maximum(W @ S, 1e-10))
            db = np.maximum(db, db.max() - 80)
            e = np.zeros(db.shape[1], dtype=np.float32)
            if db.shape[1] > F.SHIFT:
                e[F.SHIFT:] = np.maximum(0, db[:, 1:] - db[:, :-1]).mean(axis=0)[:db.shape[1] - F.SHIFT]
            masks.append(F.onset_detect(e))
        out.append(F.f1_formula(*masks))
    return out


def self_similarity_host_route(g, r, ng, nr):
    """ast_amd.mfcc on the device, one copy to the host, sklearn per clip"""
    cg, cr = M.mfcc(g, ng).cpu().numpy(), M.mfcc(r, nr).cpu().numpy()
    ngh, nrh = ng.tolist(), nr.tolist()
    return [float(np.abs(F.recurrence_sklearn(cg[b, :, :1 + ngh[b] // 512]) - F.recurrence_sklearn(cr[b, :, :1 + nrh[b] // 512])).mean())
            for b in range(cg.shape[0])]


def main():
    dev = "cuda"
    gen = torch.Generator().manual_seed(9)
    a, g = (torch.randn(len(NS), max(NS), generator=gen).to(dev) for _ in range(2))
    ng_host = [n - 256 * (i % 3) for i, n in enumerate(NS)]
    na, ng = (torch.tensor(v, dtype=torch.int32, device=dev) for v in (NS, ng_host))
    W, window = dense_filters(), torch.hann_window(2048, device=dev)
    print(f"8 clips, sections {SECTIONS}, samples {NS}; {WARM} warm-up + {REPS} timed repetitions, alternating")
    acc, ssd = M.onset_accuracy(a, g, na, ng).cpu().tolist(), M.self_similarity_distance(g, a, ng, na).cpu().tolist()
    print(f"onset_accuracy {['%.4f' % v for v in acc]}\n  host route   {['%.4f' % v for v in onsets_host_route(a, g, NS, ng_host, W, window)]}")
    print(f"self_similarity_distance {['%.4f' % v for v in ssd]}\n  host route             {['%.4f' % v for v in self_similarity_host_route(g, a, ng, na)]}")
    timed({"onset_accuracy (new kernels)": lambda: M.onset_accuracy(a, g, na, ng),
           "onset_detect alone, one batch": lambda: M.onset_detect(a, na),
           "onset_strength alone, one batch": lambda: M.onset_strength(a, na),
           "torch.stft + host chain per clip": lambda: onsets_host_route(a, g, NS, ng_host, W, window),
           "self_similarity_distance (new kernels)": lambda: M.self_similarity_distance(g, a, ng, na),
           "recurrence_matrix alone, one batch": lambda: M.recurrence_matrix(a, na),
           "mfcc alone, one batch (20, 512)": lambda: M.mfcc(a, na),
           "ast_amd.mfcc + copy + sklearn per clip": lambda: self_similarity_host_route(g, a, ng, na)})
    if "--session" in sys.argv:
        from ast_amd.infer import StyleTransferSession
        from oracle import seeded_params as sp
        ms = []
        for tag, ctor in (("content", ast_amd.ContentEncoder), ("decoder", ast_amd.Decoder)):
            m = ctor()
            m.load_state_dict(sp.seeded_state_dict(m.state_dict(), tag=tag))
            ms.append(m.to(dev).eval())
        cls = sp.seeded_normal((len(NS), 256), 7710).to(dev)
        waves = 0.1 * a
        sess = StyleTransferSession(*ms)
        timed({"transfer_and_score replay": lambda: sess.transfer_and_score(waves, cls, n_samples=na, reference=g, n_reference=ng),
               "transfer_and_score replay, onsets + self_similarity": lambda: sess.transfer_and_score(
                   waves, cls, n_samples=na, reference=g, n_reference=ng, onsets=True, self_similarity=True)})


if __name__ == "__main__":
    main()
