"""Restatement of `librosa.feature.mfcc(y, sr=22050, n_mfcc, hop_length)` with every other argument at its default, and of the
reference's mfcc_distance (evaluation_style_transfer.py:99-109), in a dtype of the caller's choice, on metrics_ref.magnitudes:

    S = |STFT|^2, n_fft 2048, centred frames, periodic Hann, T(n) = 1 + n // hop
    M = W S, W the Slaney mel filter bank: 128 x 1025, fmin 0, fmax 11025, Slaney scale and normalisation
    dB = 10 log10(max(1e-10, M)), then max(dB, max over the clip's own 128 x T values - 80)
    mfcc = the first n_mfcc rows of the orthonormal DCT-II along the mel axis
    mfcc_distance(g, r) = mean over t < min(T_g, T_r) of ||mfcc_g[:, t] - mfcc_r[:, t]||_2, each clip at its own length

float64 is what the kernels are checked against, float32 on the CPU is the rounding floor of any f32 implementation.  librosa is
not used: parity with its output is unpinned; the mel grid is pinned to the values printed in librosa.mel_frequencies' docstring
and the DCT to scipy.fft.dct (tests/test_mfcc_cpu.py).  The keyword arguments top_db, clamp_max and htk exist to seed mistakes.

Shared by tests/test_mfcc_cpu.py and tests/test_gpu_mfcc.py: the fixture, its counts and the references (once per process)."""
import functools

import numpy as np
import torch

import metrics_ref as R

SR, N_FFT, N_MELS, BINS = 22050, 2048, 128, 1025
SETTINGS = ((13, 256), (20, 512))                         # (n_mfcc, hop): mfcc_distance's call, librosa.feature.mfcc's defaults
TOP_DB, AMIN = 80.0, 1e-10

B, N_MAX = 4, 40000
COUNTS = {"constant": [40000, 20481, 2049, 1], "reflect": [40000, 20481, 2049, 1025]}            # of `original`
N_GENERATED = {"constant": [30000, 20480, 777, 300], "reflect": [30000, 20480, 1025, 1025]}


# ---- mel scale and filter bank ------------------------------------------------------------------------------------------------------
def hz_to_mel(f, htk=False):
    f = np.asarray(f, dtype=np.float64)
    if htk:
        return 2595.0 * np.log10(1.0 + f / 700.0)
    return np.where(f < 1000.0, 3.0 * f / 200.0, 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0))


def mel_to_hz(m, htk=False):
    m = np.asarray(m, dtype=np.float64)
    if htk:
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    return np.where(m < 15.0, 200.0 * m / 3.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)))


def mel_frequencies(n, fmin=0.0, fmax=SR / 2, htk=False):
    """n points, linear in mel from mel(fmin) to mel(fmax), in Hz"""
    return mel_to_hz(np.linspace(hz_to_mel(fmin, htk), hz_to_mel(fmax, htk), n), htk)


@functools.lru_cache(maxsize=None)
def mel_filters(htk=False):
    """W (128, 1025) float64"""
    mel_f = mel_frequencies(N_MELS + 2, htk=htk)
    fft_f = np.arange(BINS) * (SR / 2) / (BINS - 1)
    W = np.zeros((N_MELS, BINS))
    for i in range(N_MELS):
        lower = (fft_f - mel_f[i]) / (mel_f[i + 1] - mel_f[i])
        upper = (mel_f[i + 2] - fft_f) / (mel_f[i + 2] - mel_f[i + 1])
        W[i] = np.maximum(0.0, np.minimum(lower, upper)) * 2.0 / (mel_f[i + 2] - mel_f[i])
    return torch.from_numpy(W)


@functools.lru_cache(maxsize=None)
def dct_matrix(n_mfcc):
    """(n_mfcc, 128) float64: c_k cos(pi k (2 j + 1) / 256), c_0 = sqrt(1 / 128), c_k = sqrt(2 / 128)"""
    k = torch.arange(n_mfcc, dtype=torch.float64)[:, None]
    j = torch.arange(N_MELS, dtype=torch.float64)[None, :]
    D = torch.cos(np.pi * k * (2 * j + 1) / (2 * N_MELS)) * np.sqrt(2.0 / N_MELS)
    D[0] *= np.sqrt(0.5)
    return D


# ---- the chain ----------------------------------------------------------------------------------------------------------------------
def mel_db(x, hop, pad_mode="constant", dtype=torch.float64, htk=False):
    """10 log10(max(1e-10, W |STFT|^2)) of one clip, not yet clamped -> (128, T(n))"""
    S = R.magnitudes(x, N_FFT, hop, pad_mode, dtype) ** 2
    M = mel_filters(htk).to(dtype) @ S
    return 10 * torch.log10(torch.clamp(M, min=AMIN))


def mfcc(x, n_mfcc=20, hop=512, pad_mode="constant", dtype=torch.float64, top_db=TOP_DB, clamp_max=None, htk=False):
    """-> (n_mfcc, T(n)).  clamp_max: the maximum to clamp by instead of the clip's own (a seeded mistake); top_db None: no clamp"""
    db = mel_db(x, hop, pad_mode, dtype, htk)
    if top_db is not None:
        db = torch.maximum(db, (db.max() if clamp_max is None else clamp_max.to(dtype)) - top_db)
    return dct_matrix(n_mfcc).to(dtype) @ db


def mfcc_distance(g, r, n_mfcc=13, hop=256, pad_mode="constant", dtype=torch.float64, top_db=TOP_DB, htk=False, swap_max=False):
    """evaluation_style_transfer.py:99-109.  swap_max: each clip clamped by the OTHER clip's maximum (a seeded mistake)"""
    mg = mr = None
    if swap_max:
        mg, mr = mel_db(r, hop, pad_mode, dtype, htk).max(), mel_db(g, hop, pad_mode, dtype, htk).max()
    a, b = mfcc(g, n_mfcc, hop, pad_mode, dtype, top_db, mg, htk), mfcc(r, n_mfcc, hop, pad_mode, dtype, top_db, mr, htk)
    T = min(a.shape[1], b.shape[1])
    return ((a[:, :T] - b[:, :T]) ** 2).sum(dim=0).sqrt().mean()


# ---- the fixture ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture_waves():
    """(original, generated): two (B, N_MAX) float32 batches.  Row 0: unit-normal noise (touches neither clamp); row 1: a unit sine
    at 440 / 880 Hz over 1e-5 noise (most of its mel values sit on the top_db clamp); row 2: noise x 1.2e-6 (most of its values sit
    on the 1e-10 floor, the rest above it); row 3: noise, counts 1 and 300 (one and two frames)."""
    gen = torch.Generator().manual_seed(4200)
    a, g = torch.randn(B, N_MAX, generator=gen), torch.randn(B, N_MAX, generator=gen)
    t = torch.arange(N_MAX, dtype=torch.float64) / SR
    a[1] = torch.sin(2 * np.pi * 440 * t).float() + 1e-5 * a[1]
    g[1] = torch.sin(2 * np.pi * 880 * t).float() + 1e-5 * g[1]
    a[2] *= 1.2e-6
    g[2] *= 1.2e-6
    return a, g


def clips(pad_mode):
    """[(original clip, generated clip)] per row, each at its own count"""
    a, g = fixture_waves()
    return [(a[b, :COUNTS[pad_mode][b]], g[b, :N_GENERATED[pad_mode][b]]) for b in range(B)]


def _evaluate(pad_mode, n_mfcc, hop, dtype):
    out = dict(orig=[], gen=[], dist=[])
    for x, y in clips(pad_mode):
        out["orig"].append(mfcc(x, n_mfcc, hop, pad_mode, dtype))
        out["gen"].append(mfcc(y, n_mfcc, hop, pad_mode, dtype))
        out["dist"].append(mfcc_distance(y, x, n_mfcc, hop, pad_mode, dtype))
    out["dist"] = torch.stack(out["dist"])
    return out


@functools.lru_cache(maxsize=None)
def references(pad_mode, n_mfcc, hop):
    """float64: dict(orig, gen: per row (n_mfcc, T_b) of the two batches; dist (B,) = mfcc_distance(generated, original);
    peak_orig, peak_gen: per row the clip's peak |coefficient|; peak_pair: the larger of the two)"""
    ref = _evaluate(pad_mode, n_mfcc, hop, torch.float64)
    ref["peak_orig"] = [float(m.abs().max()) for m in ref["orig"]]
    ref["peak_gen"] = [float(m.abs().max()) for m in ref["gen"]]
    ref["peak_pair"] = [max(p, q) for p, q in zip(ref["peak_orig"], ref["peak_gen"])]
    return ref


def coef_error(got, ref, which, b):
    """largest absolute error over clip b's coefficients, relative to the clip's peak |coefficient|"""
    return float((got.double() - ref[which][b]).abs().max()) / ref["peak_" + which][b]


def dist_error(got, ref, b):
    """absolute error of pair b's distance relative to the pair's peak |coefficient|: the distance inherits the coefficients'
    absolute error, and on row 2 it is far smaller than they are, so an error relative to the distance itself would measure
    cancellation"""
    return abs(float(got) - float(ref["dist"][b])) / ref["peak_pair"][b]


@functools.lru_cache(maxsize=None)
def f32_floor(pad_mode):
    """The rounding floor: the restatement in float32 on the CPU against its float64 form, maximum over rows, batches and SETTINGS"""
    coef = dist = 0.0
    for n_mfcc, hop in SETTINGS:
        ref, f32 = references(pad_mode, n_mfcc, hop), _evaluate(pad_mode, n_mfcc, hop, torch.float32)
        for b in range(B):
            coef = max(coef, coef_error(f32["orig"][b], ref, "orig", b), coef_error(f32["gen"][b], ref, "gen", b))
            dist = max(dist, dist_error(f32["dist"][b], ref, b))
    return dict(coef=coef, dist=dist)


def bounds(pad_mode):
    """the project's rule: 10 x the float32 floor"""
    return {k: 10 * v for k, v in f32_floor(pad_mode).items()}
