"""Restatement of librosa's documented chain for piptrack, estimate_tuning, filters.chroma and feature.chroma_stft, and of the
reference's chroma_distance (evaluation_reconstruction.py:39-52), pitch_correlation (:83-103) and chroma_similarity
(evaluation_style_transfer.py:80-96), in NumPy in a dtype of the caller's choice, on metrics_ref.magnitudes (sr = 22 050):

    piptrack(S), fmin 150, fmax 4000, threshold 0.1: for 0 < k < K - 1, avg = (S[k+1] - S[k-1]) / 2, den = 2 S[k] - S[k+1] - S[k-1],
        shift = avg / (den + (|den| < tiny)), dskew = avg shift / 2; bin k is a peak of frame t if 150 <= k sr / n_fft < 4000,
        S[k] > 0.1 max_k S, S[k] > S[k-1], S[k] >= S[k+1]; there pitch = (k + shift) sr / n_fft, mag = S[k] + dskew, else both 0
    estimate_tuning(S = |STFT|^2): the peaks with mag >= median(mag); r = frac(12 log2(pitch / 27.5)), wrapped to [-0.5, 0.5);
        np.histogram over linspace(-0.5, 0.5, 101); tuning = the left edge of the fullest bin (the lowest wins ties), 0.0 without a peak
    filters.chroma(sr, n_fft, tuning): q[k] = 12 log2(f_k / 27.5) - tuning, q[0] = q[1] - 18, width[k] = max(q[k+1] - q[k], 1),
        D[c, k] = ((q[k] - c + 126) mod 12) - 6, w = exp(-(2 D / width)^2 / 2), every column to unit L2 norm, times
        exp(-((q / 12 - 5) / 2)^2 / 2), rows rolled by -3 (row 0 = C)
    chroma_stft: w |STFT|^2, every frame divided by its maximum unless that is below float32 tiny
    pitch_mean: the mean over all K bins of piptrack(|STFT|)'s pitches, per frame

float64 is what the kernels are checked against, float32 (the same code) is the rounding floor of any f32 implementation.
librosa is not used: parity with its own output is unpinned.  Shared by tests/test_chroma_cpu.py and tests/test_gpu_chroma.py: the
fixture, its counts and the references (once per process)."""
import functools
import warnings

import numpy as np
import scipy.stats
import torch

import metrics_ref as R

SR = 22050
WIDE, NARROW = (2048, 512), (1024, 256)                   # librosa's defaults (chroma_distance, pitch_correlation); chroma_similarity's call
F32_TINY = float(np.finfo(np.float32).tiny)

B, N_MAX = 4, 12000
COUNTS = [12000, 8000, 3800, 3900]                        # of `original`; every count reflect-pads at n_fft 2048 (>= 1025)
N_GENERATED = [9000, 8100, 3000, 7777]


def _tdtype(dtype):
    return torch.float64 if np.dtype(dtype) == np.float64 else torch.float32


def spectrum(x, n_fft, hop, pad_mode="constant", dtype=np.float64, power=True):
    """|STFT| or |STFT|^2 of one clip -> (K, T) in `dtype`"""
    S = R.magnitudes(x, n_fft, hop, pad_mode, _tdtype(dtype))
    return (S ** 2 if power else S).numpy()


def band(n_fft):
    """the first and the last bin with 150 <= k sr / n_fft < 4000"""
    f = np.arange(1 + n_fft // 2) * SR / n_fft
    k = np.flatnonzero((f >= 150) & (f < 4000))
    return int(k[0]), int(k[-1])


def piptrack(S, n_fft):
    """-> (pitch, mag), both (K, T) in S's dtype"""
    dt = S.dtype
    K = S.shape[0]
    avg = dt.type(0.5) * (S[2:] - S[:-2])
    den = dt.type(2) * S[1:-1] - S[2:] - S[:-2]
    shift = avg / (den + (np.abs(den) < np.finfo(dt).tiny))
    dskew = dt.type(0.5) * avg * shift
    lo, hi = band(n_fft)
    k = np.arange(K, dtype=dt)[:, None]
    peak = np.zeros(S.shape, dtype=bool)
    peak[1:-1] = (S[1:-1] > dt.type(0.1) * S.max(axis=0)) & (S[1:-1] > S[:-2]) & (S[1:-1] >= S[2:])
    peak[:lo] = False
    peak[hi + 1:] = False
    pitch, mag = np.zeros_like(S), np.zeros_like(S)
    pitch[1:-1] = (k[1:-1] + shift) * dt.type(SR) / dt.type(n_fft)
    mag[1:-1] = S[1:-1] + dskew
    return np.where(peak, pitch, 0).astype(dt), np.where(peak, mag, 0).astype(dt)


def tuning_info(S, n_fft):
    """estimate_tuning on a power spectrogram -> dict(tuning, n: peaks, kept, thr, hist (100,))"""
    pitch, mag = piptrack(S, n_fft)
    cand = pitch > 0
    n = int(cand.sum())
    if n == 0:
        return dict(tuning=0.0, n=0, kept=0, thr=0.0, hist=np.zeros(100, dtype=np.int64))
    thr = np.median(mag[cand])
    keep = cand & (mag >= thr)
    r = np.mod(S.dtype.type(12) * np.log2(pitch[keep] / S.dtype.type(27.5)), S.dtype.type(1))
    r[r >= 0.5] -= 1
    edges = np.linspace(-0.5, 0.5, 101)
    hist, _ = np.histogram(r, bins=edges)
    return dict(tuning=float(edges[int(np.argmax(hist))]), n=n, kept=int(keep.sum()), thr=float(thr), hist=hist)


def estimate_tuning(x, n_fft=2048, hop=512, pad_mode="constant", dtype=np.float64):
    return tuning_info(spectrum(x, n_fft, hop, pad_mode, dtype), n_fft)["tuning"]


def chroma_filters(n_fft, tuning=0.0, dtype=np.float64, octave=True):
    """(12, K) in `dtype`; octave=False: without the octave weighting"""
    dt = np.dtype(dtype).type
    K = 1 + n_fft // 2
    f = (np.arange(1, K + 1) * SR / n_fft).astype(dtype)
    q = np.empty(K + 1, dtype=dtype)
    q[1:] = dt(12) * np.log2(f / dt(27.5)) - dt(tuning)
    q[0] = q[1] - dt(18)
    width = np.maximum(q[1:] - q[:-1], dt(1))
    q = q[:K]
    D = np.mod(q[None, :] - np.arange(12, dtype=dtype)[:, None] + dt(126), dt(12)) - dt(6)
    w = np.exp(dt(-0.5) * (dt(2) * D / width) ** 2)
    w = w / np.sqrt((w * w).sum(axis=0))
    if octave:
        w = w * np.exp(dt(-0.5) * ((q / dt(12) - dt(5)) / dt(2)) ** 2)
    return np.roll(w, -3, axis=0).astype(dtype)


def chroma_stft(x, n_fft=2048, hop=512, pad_mode="constant", dtype=np.float64, tuning=None):
    """-> (12, T(n)) in `dtype`; tuning None: the clip's own estimate"""
    S = spectrum(x, n_fft, hop, pad_mode, dtype)
    if tuning is None:
        tuning = tuning_info(S, n_fft)["tuning"]
    raw = chroma_filters(n_fft, tuning, dtype) @ S
    mx = np.abs(raw).max(axis=0)
    return raw / np.where(mx < F32_TINY, 1, mx).astype(dtype)


def pearson(x, y):
    """scipy.stats.pearsonr's r; nan where it is not defined (fewer than 2 values, a constant vector)"""
    if len(x) < 2:
        return float("nan")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return float(scipy.stats.pearsonr(x, y)[0])


def chroma_distance(o, g, pad_mode="constant", dtype=np.float64):
    L = min(len(o), len(g))
    co, cg = (chroma_stft(x[:L], *WIDE, pad_mode, dtype) for x in (o, g))
    return float(np.sqrt(((co - cg) ** 2).sum(axis=0)).mean())


def chroma_similarity(g, o, pad_mode="constant", dtype=np.float64):
    cg, co = (chroma_stft(x, *NARROW, pad_mode, dtype) for x in (g, o))
    T = min(cg.shape[1], co.shape[1])
    r = [pearson(cg[c, :T], co[c, :T]) for c in range(12)]
    r = [v for v in r if np.isfinite(v)]
    return float(np.mean(r)) if r else 0.0


def pitch_mean(x, pad_mode="constant", dtype=np.float64):
    """-> (T(n),) in `dtype`"""
    return piptrack(spectrum(x, *WIDE, pad_mode, dtype, power=False), WIDE[0])[0].mean(axis=0)


def pitch_correlation(o, g, pad_mode="constant", dtype=np.float64):
    L = min(len(o), len(g))
    r = pearson(pitch_mean(o[:L], pad_mode, dtype), pitch_mean(g[:L], pad_mode, dtype))
    return r if np.isfinite(r) else 0.0


# ---- the fixture ----------------------------------------------------------------------------------------------------------------------
TONES = ((8, 21, 12), (7, 17, 12), (9, 21, 8), (17, 21, 12))   # per clip: the fundamentals of its three tones, in bins of n_fft 1024


def tones(fundamentals, seed, n=N_MAX, shift=0.0):
    """Three harmonic tones (the partials 1, 2, 4, ... below 4 kHz) over 1e-3 noise -> (n,) float32.  The fundamentals sit on
    bin centres of n_fft 1024 (and so of 2048), where piptrack's parabola has no bias, and are detuned from equal temperament by
    what that gives: -0.234 semitones for bin 8, +0.454 for 7, -0.195 for 9, -0.185 for 17, each well inside a bin of the tuning
    histogram.  The first tone is the loudest and steady, so its partials are the peaks above the median; the other two are gated
    by slow envelopes of their own, so that the frames' peak sets, mean pitches and chroma rows move over the clip.
    shift: every tone raised by that many semitones."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    x = np.zeros(n)
    for i, k0 in enumerate(fundamentals):
        k = k0
        while k * SR / 1024 < 4000:
            f = k * SR / 1024 * 2 ** (shift / 12)
            env = 0.45 * np.clip(0.5 + 1.5 * np.sin(2 * np.pi * (rng.uniform(2.0, 5.0) * t + rng.uniform())), 0, 1) if i else rng.uniform(0.9, 1.0)
            x += env * np.sin(2 * np.pi * (f * t + rng.uniform()))
            k *= 2
    return (x / 8 + 1e-3 * rng.standard_normal(n)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def fixture_waves(shift=0.0):
    """(original, generated): two (B, N_MAX) float32 batches; `generated` is the same tones under other envelopes and noise, at 0.8 of the level"""
    a = np.stack([tones(TONES[b], 100 + b, shift=shift) for b in range(B)])
    g = np.stack([0.8 * tones(TONES[b], 200 + b, shift=shift) for b in range(B)])
    return torch.from_numpy(a), torch.from_numpy(g)


def clips():
    """[(original clip, generated clip)] per row, each at its own count"""
    a, g = fixture_waves()
    return [(a[b, :COUNTS[b]], g[b, :N_GENERATED[b]]) for b in range(B)]


def _evaluate(pad_mode, dtype, tunings=None):
    """tunings: per setting, row and batch the tuning to build the chroma with (None: the clip's own estimate)"""
    out = dict(pitch=[], dist=[], sim=[], corr=[])
    for s in (WIDE, NARROW):
        out["info", s] = [[tuning_info(spectrum(x, *s, pad_mode, dtype), s[0]) for x in pair] for pair in clips()]
        use = tunings[s] if tunings else [[i["tuning"] for i in row] for row in out["info", s]]
        out["chroma", s] = [[chroma_stft(x, *s, pad_mode, dtype, tuning=use[b][j]) for j, x in enumerate(pair)]
                            for b, pair in enumerate(clips())]
    for o, g in clips():
        out["pitch"].append([pitch_mean(o, pad_mode, dtype), pitch_mean(g, pad_mode, dtype)])
        out["dist"].append(chroma_distance(o, g, pad_mode, dtype))
        out["sim"].append(chroma_similarity(g, o, pad_mode, dtype))
        out["corr"].append(pitch_correlation(o, g, pad_mode, dtype))
    return out


@functools.lru_cache(maxsize=None)
def references(pad_mode):
    """float64: dict(("info", setting): per row and batch tuning_info; ("chroma", setting): per row and batch (12, T_b) at the
    clip's own tuning; pitch: per row and batch (T_b,); dist, sim, corr: (B,) lists)"""
    return _evaluate(pad_mode, np.float64)


@functools.lru_cache(maxsize=None)
def twin(pad_mode):
    """the same in float32, with the float64 tunings supplied to its chroma_stft (its own estimates are in its info)"""
    ref = references(pad_mode)
    return _evaluate(pad_mode, np.float32, {s: [[i["tuning"] for i in row] for row in ref["info", s]] for s in (WIDE, NARROW)})


def peak_error(got, want):
    """largest absolute error relative to the clip's peak value"""
    want = np.asarray(want, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / np.abs(want).max())


@functools.lru_cache(maxsize=None)
def f32_floor(pad_mode):
    """The rounding floor: the float32 twin against float64, maximum over rows and batches.  chroma and pitch: relative to the
    clip's peak value; thr: relative to the median itself; dist, sim, corr: absolute (the scores are of order 1)."""
    ref, f32 = references(pad_mode), twin(pad_mode)
    fl = dict(chroma=0.0, pitch=0.0, thr=0.0)
    for b in range(B):
        for j in range(2):
            fl["pitch"] = max(fl["pitch"], peak_error(f32["pitch"][b][j], ref["pitch"][b][j]))
            for s in (WIDE, NARROW):
                fl["chroma"] = max(fl["chroma"], peak_error(f32["chroma", s][b][j], ref["chroma", s][b][j]))
                fl["thr"] = max(fl["thr"], abs(f32["info", s][b][j]["thr"] - ref["info", s][b][j]["thr"]) / ref["info", s][b][j]["thr"])
    for k in ("dist", "sim", "corr"):
        fl[k] = max(abs(x - y) for x, y in zip(f32[k], ref[k]))
    return fl


def bounds(pad_mode):
    """the project's rule: 10 x the float32 floor"""
    return {k: 10 * v for k, v in f32_floor(pad_mode).items()}


def allowance(pad_mode, s, b, j):
    """A = max(4, 10 x the L1 distance of the twin's histogram from the float64 one): what a float32 implementation may move"""
    return max(4, 10 * int(np.abs(twin(pad_mode)["info", s][b][j]["hist"] - references(pad_mode)["info", s][b][j]["hist"]).sum()))
