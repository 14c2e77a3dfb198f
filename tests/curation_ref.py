"""Restatement of what the reference's dataset screening scripts (Preprocessing_Dataset/) compute, from librosa's and pydub's
documented definitions, in float64 NumPy:

    frame_rms       librosa.feature.rms(y)[0]: frame_length 2048, hop_length 512, center=True -- the clip padded by 1024 samples at
                    both ends ("constant": zeros; "reflect": mirrored without the edge sample), cut into T = 1 + n // 512 frames of
                    2048 samples 512 apart, rms[t] = sqrt(mean(frame_t ** 2))                      (silent_tracks_dataset.py:20-27)
    silent_frames   sum(rms < 0.005); silence_ratio = silent_frames / T; a track is flagged at >= 0.3
    clip_rms        sqrt(mean(y ** 2))                                                          (dataset_tracks_analysis.py:27)
    mfcc_mean       mean(librosa.feature.mfcc(y, sr, n_mfcc=13), axis=1): mfcc_ref's chain with the mel filter bank built for the
                    clip's own rate, the DCT taken per frame, then the mean over the frames (:28-29; dataset_variety.py:13-16)
    rms_normalize   y * (target / clip_rms), y itself where clip_rms == 0                        (unifies_violin_datasets.py:25-30)
    sound_windows   is_mostly_sound's rule: windows of win = sr // 10 samples, W = n // win of them, a window sounds when
                    20 log10(sqrt(mean(window ** 2))) > -45 at full scale 1.0, never when its level is 0; sound_ratio = sounding / W,
                    0 when W = 0; a clip is kept at >= 0.6                                       (split_BachViolinDataset.py:24-30)

and a float32 twin (twin_*) that follows the kernels' summation orders (csrc/curation.hip): hop blocks of 512 samples, lane l of a
wave squaring the samples 4 l .. 4 l + 3 and 256 + 4 l .. of a block in a fixed tree, the wave sum's exchange order, four block sums
per frame ascending; block sums added in double for the level; the clamped float32 dB rows added per 32-frame chunk in float32, the
chunks in double, one DCT of the mean in double.  The twin's error against float64 is the rounding floor of the device results; 10 x
that floor is the bound of tests/test_gpu_curation.py.  librosa and pydub are not used: parity with their own output is unpinned.

Shared by tests/test_curation_cpu.py and tests/test_gpu_curation.py: the fixture, its counts and the references (once per process)."""
import functools

import numpy as np
import torch

import metrics_ref as R
import mfcc_ref as MR

FRAME, HOP = 2048, 512
TILE, CHUNK = 32, 32                                     # ast_frame_rms_tile_frames, ast_mfcc_mean_chunk_frames (asserted in the CPU test)
SILENCE_RMS, SOUND_DB, TARGET_RMS = 0.005, -45.0, 0.07
N_MFCC = 13
RATES = (22050, 44100)
MODES = ("constant", "reflect")

N_MAX = 2 * TILE * HOP + 1000                            # 33 768: a little over two tiles of frames (66 frames, three tiles)
ZERO_ROW, MIX_ROW = 10, 11
COUNTS = {"constant": [1, 511, 512, 2047, 2048, 2049, TILE * HOP - 1, TILE * HOP, TILE * HOP + 1, N_MAX, 20000, 30000],
          "reflect": [1025, 1026, 1535, 2047, 2048, 2049, TILE * HOP - 1, TILE * HOP, TILE * HOP + 1, N_MAX, 20000, 30000]}
B = len(COUNTS["constant"])
LOUD, QUIET = 0.02, 0.001                                # sine amplitudes of the mixed clip
# per hop block, cyclic: a de Bruijn sequence, so that a run of four blocks (a frame) takes each of the 16 loud / quiet mixes, then a
# quiet stretch longer than two 100 ms windows at 44 100 Hz
PATTERN = [0, 0, 0, 0, 1, 0, 0, 1, 1, 0, 1, 0, 1, 1, 1, 1] + [0] * 12


def n_frames(n):
    return 1 + n // HOP


@functools.lru_cache(maxsize=None)
def fixture_waves():
    """(B, N_MAX) float32.  Rows 0 .. 9: 0.1 x unit-normal noise plus a 0.05 sine at 440 Hz, at the counts where the kernels take
    another path (one sample, around a hop block, around a frame, the last frame of a tile, the first of the next, the full row);
    row 10: zeros; row 11: a 441 Hz sine whose amplitude is LOUD or QUIET per hop block after PATTERN."""
    gen = torch.Generator().manual_seed(5150)
    w = 0.1 * torch.randn(B, N_MAX, generator=gen)
    t = torch.arange(N_MAX, dtype=torch.float64)
    w += (0.05 * torch.sin(2 * np.pi * 440 * t / 22050)).float()
    w[ZERO_ROW] = 0
    amp = torch.tensor([LOUD if PATTERN[(i // HOP) % len(PATTERN)] else QUIET for i in range(N_MAX)], dtype=torch.float64)
    w[MIX_ROW] = (amp * torch.sin(2 * np.pi * 441 * t / 22050)).float()
    return w


def clips(pad_mode):
    w = fixture_waves().numpy()
    return [w[b, :COUNTS[pad_mode][b]] for b in range(B)]


# ---- float64: the definitions ---------------------------------------------------------------------------------------------------------
def padded(x, pad_mode):
    x = np.asarray(x)
    return np.pad(x, FRAME // 2, mode="reflect") if pad_mode == "reflect" else np.pad(x, FRAME // 2)


def frames(x, pad_mode):
    """(T, 2048): explicit padding and framing"""
    return np.lib.stride_tricks.sliding_window_view(padded(x, pad_mode), FRAME)[::HOP]


def frame_rms(x, pad_mode="constant"):
    fr = frames(np.asarray(x, dtype=np.float64), pad_mode)
    assert fr.shape[0] == n_frames(len(x))
    return np.sqrt(np.mean(fr ** 2, axis=1))


def silent_frames(x, pad_mode="constant", threshold=SILENCE_RMS):
    return int(np.sum(frame_rms(x, pad_mode) < threshold))


def clip_rms(x):
    return float(np.sqrt(np.mean(np.asarray(x, dtype=np.float64) ** 2)))


def window_levels(x, sample_rate, frame_ms=100):
    """(W,) the level of every whole window"""
    win = sample_rate * frame_ms // 1000
    x = np.asarray(x, dtype=np.float64)
    W = len(x) // win
    return np.sqrt(np.mean(x[:W * win].reshape(W, win) ** 2, axis=1)) if W else np.zeros(0)


def level_db(r):
    with np.errstate(divide="ignore"):
        return 20 * np.log10(r)


def sound_windows(x, sample_rate, threshold_db=SOUND_DB):
    r = window_levels(x, sample_rate)
    return ((r > 0) & (level_db(r) > threshold_db)).astype(np.int32)


def sound_ratio(x, sample_rate, threshold_db=SOUND_DB):
    m = sound_windows(x, sample_rate, threshold_db)
    return float(m.sum() / len(m)) if len(m) else 0.0


@functools.lru_cache(maxsize=None)
def mel_filters(sample_rate):
    """librosa.filters.mel(sr, 2048, n_mels=128) as documented: Slaney scale and normalisation, fmin 0, fmax sr / 2 -> (128, 1025) float64"""
    mel_f = MR.mel_frequencies(MR.N_MELS + 2, fmax=sample_rate / 2)
    fft_f = np.arange(MR.BINS) * (sample_rate / 2) / (MR.BINS - 1)
    W = np.zeros((MR.N_MELS, MR.BINS))
    for i in range(MR.N_MELS):
        lower = (fft_f - mel_f[i]) / (mel_f[i + 1] - mel_f[i])
        upper = (mel_f[i + 2] - fft_f) / (mel_f[i + 2] - mel_f[i + 1])
        W[i] = np.maximum(0.0, np.minimum(lower, upper)) * 2.0 / (mel_f[i + 2] - mel_f[i])
    return torch.from_numpy(W)


def mel_db(x, sample_rate, hop=HOP, pad_mode="constant", dtype=torch.float64):
    """the clamped dB rows (128, T) in `dtype`"""
    S = R.magnitudes(torch.as_tensor(np.asarray(x)), FRAME, hop, pad_mode, dtype) ** 2
    db = 10 * torch.log10(torch.clamp(mel_filters(sample_rate).to(dtype) @ S, min=MR.AMIN))
    return torch.maximum(db, db.max() - MR.TOP_DB)


def mfcc_frames(x, sample_rate, n_mfcc=N_MFCC, hop=HOP, pad_mode="constant"):
    """(n_mfcc, T) float64: the DCT of every frame"""
    return (MR.dct_matrix(n_mfcc) @ mel_db(x, sample_rate, hop, pad_mode)).numpy()


def mfcc_mean(x, sample_rate, n_mfcc=N_MFCC, hop=HOP, pad_mode="constant"):
    """the mean of the per-frame DCT"""
    return mfcc_frames(x, sample_rate, n_mfcc, hop, pad_mode).mean(axis=1)


def rms_normalize(x, target=TARGET_RMS):
    x = np.asarray(x, dtype=np.float64)
    level = clip_rms(x)
    return x if level == 0 else x * (target / level)


# ---- float32: the kernels' orders ---------------------------------------------------------------------------------------------------
_L = np.arange(64)
_ROR4 = (_L & 48) | ((_L - 4) & 15)
_ROR8 = (_L & 48) | ((_L - 8) & 15)


def _wave_sum(v):
    """(..., 64) float32 -> (...): quad swaps, row rotations by 4 and 8, then the four rows (ast_common.h wave_sum_dpp)"""
    v = v + v[..., _L ^ 1]
    v = v + v[..., _L ^ 2]
    v = v + v[..., _ROR4]
    v = v + v[..., _ROR8]
    return (v[..., 0] + v[..., 16]) + (v[..., 32] + v[..., 48])


def _block_sums(blocks):
    """(nb, 512) float32 -> (nb,) float32"""
    q = (blocks * blocks).reshape(-1, 2, 64, 4)                                        # [block][half][lane][i]
    h = (q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])
    return _wave_sum(h[:, 0] + h[:, 1])


def twin_blocks(x, pad_mode):
    """-> (padded sums of the hop blocks -2 .. T, own sums of the blocks 0 .. T - 1), float32"""
    x = np.asarray(x, dtype=np.float32)
    T = n_frames(len(x))
    p = padded(x, pad_mode)[:(T + 3) * HOP]                                            # n + 2048 >= 512 (T + 3); behind frame T - 1 nothing is used
    own = np.concatenate([x, np.zeros(T * HOP - len(x), dtype=np.float32)])
    return _block_sums(p.reshape(-1, HOP)), _block_sums(own.reshape(-1, HOP))


def twin_frame_rms(x, pad_mode="constant"):
    bs, _ = twin_blocks(x, pad_mode)
    T = n_frames(len(x))
    ss = ((bs[0:T] + bs[1:T + 1]) + bs[2:T + 2]) + bs[3:T + 3]
    return np.sqrt(ss * np.float32(1 / FRAME))


def twin_sumsq(x, pad_mode="constant"):
    """the clip's own sum of squares as the kernels add it: block sums ascending in double per tile, the tiles ascending"""
    _, us = twin_blocks(x, pad_mode)
    s = 0.0
    for t0 in range(0, len(us), TILE):
        part = 0.0
        for v in us[t0:t0 + TILE]:
            part += float(v)
        s += part
    return s


def twin_clip_rms(x):
    return np.float32(np.sqrt(twin_sumsq(x) / len(x)))


def twin_mfcc_mean(x, sample_rate, n_mfcc=N_MFCC, hop=HOP, pad_mode="constant"):
    db = mel_db(x, sample_rate, hop, pad_mode, torch.float32).numpy().T                # (T, 128) float32
    T = db.shape[0]
    total = np.zeros(MR.N_MELS)
    for t0 in range(0, T, CHUNK):
        s = np.zeros(MR.N_MELS, dtype=np.float32)
        for row in db[t0:t0 + CHUNK]:
            s = s + row
        total += s.astype(np.float64)
    return (MR.dct_matrix(n_mfcc).numpy() @ (total / T)).astype(np.float32)


def twin_rms_normalize(x, target=TARGET_RMS):
    x = np.asarray(x, dtype=np.float32)
    level = np.sqrt(twin_sumsq(x) / len(x))
    return x * (np.float32(target / level) if level > 0 else np.float32(1))


# ---- references, errors and bounds --------------------------------------------------------------------------------------------------
def _evaluate(pad_mode, twin):
    out = dict(rms=[], level=[], norm=[], mfcc={sr: [] for sr in RATES})
    for x in clips(pad_mode):
        out["rms"].append(twin_frame_rms(x, pad_mode) if twin else frame_rms(x, pad_mode))
        out["level"].append(float(twin_clip_rms(x)) if twin else clip_rms(x))
        out["norm"].append(twin_rms_normalize(x) if twin else rms_normalize(x))
        for sr in RATES:
            out["mfcc"][sr].append(twin_mfcc_mean(x, sr, pad_mode=pad_mode) if twin else mfcc_mean(x, sr, pad_mode=pad_mode))
    return out


@functools.lru_cache(maxsize=None)
def references(pad_mode):
    """float64 per row: rms (T_b,), level, norm (n_b,), mfcc[sr] (13,); and the integer results: silent, sound[sr] (W_b,) masks"""
    ref = _evaluate(pad_mode, False)
    ref["silent"] = [silent_frames(x, pad_mode) for x in clips(pad_mode)]
    ref["sound"] = {sr: [sound_windows(x, sr) for x in clips(pad_mode)] for sr in RATES}
    return ref


def rel_peak(got, ref):
    """largest absolute error relative to the reference's peak magnitude; where the reference is all zero, the largest absolute value"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    peak = float(np.abs(ref).max())
    return float(np.abs(got - ref).max()) / (peak if peak > 0 else 1.0)


def errors(got, pad_mode):
    """got: rows like references(pad_mode) -> dict(rms, level, norm, mfcc): the largest rel_peak over the rows (and the rates)"""
    ref = references(pad_mode)
    e = {k: max(rel_peak(g, r) for g, r in zip(got[k], ref[k])) for k in ("rms", "level", "norm")}
    e["mfcc"] = max(rel_peak(g, r) for sr in RATES for g, r in zip(got["mfcc"][sr], ref["mfcc"][sr]))
    return e


@functools.lru_cache(maxsize=None)
def f32_floor(pad_mode):
    """the float32 twin against float64"""
    return errors(_evaluate(pad_mode, True), pad_mode)


def bounds(pad_mode):
    """the project's rule: 10 x the float32 floor"""
    return {k: 10 * v for k, v in f32_floor(pad_mode).items()}
