"""Spectrogram metrics of the reference's evaluation scripts on the device, for a padded batch of clips of different lengths:

    mse_spectrogram            evaluation_reconstruction.py:105-118 (on the audio truncated to a common length, :193-204)
    instrumentation_similarity evaluation_style_transfer.py:111-119 (band energies + Pearson's r)

    mfcc, mfcc_distance        evaluation_style_transfer.py:99-109: librosa.feature.mfcc restated as a formula chain (below)
    chroma_distance, pitch_correlation   evaluation_reconstruction.py:39-52, 83-103 \  librosa's piptrack, estimate_tuning, filters.chroma
    chroma_similarity                    evaluation_style_transfer.py:80-96         /  and chroma_stft restated (csrc/chroma.hip, below)
    onset_accuracy             evaluation_reconstruction.py:54-81: librosa.onset.onset_detect restated, then the F1 score (below)
    self_similarity_distance   evaluation_style_transfer.py:121-133: librosa.segment.recurrence_matrix(mfcc.T) restated (below)

All are |STFT| plus a reduction (csrc/metrics.hip); the spectrogram is never stored and no length is read on the host, so the
calls can be captured in a graph (StyleTransferSession.transfer_and_score).  `librosa.stft`'s documented defaults are restated,
not linked: centred frames, periodic Hann window, T(n) = 1 + n // hop frames; pad_mode "constant" (librosa >= 0.10, the default)
or "reflect" (librosa < 0.10, get_STFT).  Parity with librosa's own output is unpinned ("Spectrogram metrics")."""
from __future__ import annotations

import ctypes

import torch

from ._lib import check, len_tensor, lib, ptr, stream

PAD_MODES = {"constant": 0, "reflect": 1}
MSE_N_FFT, MSE_HOP = 1024, 256                           # N_FFT, HOP_LENGTH of evaluation_reconstruction.py
BAND_N_FFT, BAND_HOP, BAND_BINS = 2048, 512, 1025        # librosa.stft defaults
MFCC_N_FFT, MFCC_SR, MFCC_HOPS = 2048, 22050, (256, 512)  # librosa.feature.mfcc defaults; HOP_LENGTH of the two evaluation scripts


def _rows(t, name, what, n_fft, pad_mode):
    if pad_mode not in PAD_MODES:
        raise ValueError(f"{name}: pad_mode must be 'constant' or 'reflect', got {pad_mode!r}")
    if not torch.is_tensor(t) or t.dim() != 2 or t.dtype != torch.float32 or t.shape[0] < 1 or t.shape[1] < 1:
        got = f"{t.dtype} {tuple(t.shape)}" if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"{name}: {what} must be (B, n) float32 rows, got {got}")
    if pad_mode == "reflect" and t.shape[1] < n_fft // 2 + 1:
        raise ValueError(f"{name}: reflect padding needs rows of at least {n_fft // 2 + 1} samples, {what} has {t.shape[1]}")
    return t.contiguous()


def _one(name, waves, n_samples, n_fft, pad_mode):
    """the rows and counts of one batch, checked"""
    w = _rows(waves, name, "waves", n_fft, pad_mode)
    return w, len_tensor(n_samples, w.shape[0], "n_samples", device=True, contiguous=True)


def _pair(name, a, what_a, b, what_b, n_a, n_b, n_fft, pad_mode):
    """the rows and counts of a pair of batches, checked"""
    a, b = _rows(a, name, what_a, n_fft, pad_mode), _rows(b, name, what_b, n_fft, pad_mode)
    B = a.shape[0]
    if b.shape[0] != B:
        raise ValueError(f"{name}: {B} {what_a} and {b.shape[0]} {what_b} rows")
    return a, b, len_tensor(n_a, B, "n_" + what_a, device=True, contiguous=True), len_tensor(n_b, B, "n_" + what_b, device=True, contiguous=True)


_mel_tables = {}


def _mel_table(device, sample_rate):
    """The Slaney mel filter bank at `sample_rate` as the sparse table the kernels read (ast_mel_table: built on the host in double),
    on `device`; one per (device, sample_rate).  Filled on first use, which has to happen outside a graph capture: a session's
    warm-up runs do that."""
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device(), sample_rate)
    if key not in _mel_tables:
        L = lib()
        words = (ctypes.c_int32 * L.ast_mel_table_words())()
        check(L.ast_mel_table(sample_rate, ctypes.addressof(words)), "ast_mel_table")
        _mel_tables[key] = torch.tensor(list(words), dtype=torch.int32).to(device)
    return _mel_tables[key]


def _run(entry, rows, counts, outs, pad_mode, extra=(), ws_extra=(), sample_rate=None):
    """The call of ast_<entry>_len on one batch or on the two of a pair (rows, counts: one or two checked tensors each), in the order
    of its refusals: a host tensor first, then the mel table at `sample_rate` (None: the entry takes none), then the workspace of
    ast_<entry>_ws_floats(B, row widths, *ws_extra) and the outputs -- outs: (shape, dtype) each, or None for a null pointer.
    extra: the entry's arguments between the counts and the pad mode.  -> the list of outputs"""
    L = lib()
    B, dev, widths = rows[0].shape[0], rows[0].device, [t.shape[1] for t in rows]
    p = [ptr(t) for t in rows]
    table = () if sample_rate is None else (ptr(_mel_table(dev, sample_rate)),)
    ws = torch.empty(getattr(L, f"ast_{entry}_ws_floats")(B, *widths, *ws_extra), dtype=torch.float32, device=dev)
    outs = [o and torch.empty(o[0], dtype=o[1], device=dev) for o in outs]
    front = (p[0], B, widths[0], ptr(counts[0])) if len(rows) == 1 else (p[0], widths[0], p[1], widths[1], B, ptr(counts[0]), ptr(counts[1]))
    check(getattr(L, f"ast_{entry}_len")(*front, *extra, PAD_MODES[pad_mode], *table, ptr(ws), ws.numel(), *map(ptr, outs), stream()),
          f"ast_{entry}_len")
    return outs


def mse_spectrogram(original, generated, n_original=None, n_generated=None, pad_mode="constant"):
    """original (B, n), generated (B, m) f32 device rows -> (B,) f32: mean over 513 x T_b of (|A| - |G|)^2 at n_fft 1024, hop 256,
    both clips cut to L_b = min(n_original[b], n_generated[b]) samples first, T_b = 1 + L_b // 256.
    n_original, n_generated: int32 (B,) device tensors, clamped on the device to [1, row width] ([513, row width] with
    pad_mode="reflect"); None: the rows are full."""
    a, g, na, ng = _pair("mse_spectrogram", original, "original", generated, "generated", n_original, n_generated, MSE_N_FFT, pad_mode)
    return _run("spec_mse", (a, g), (na, ng), [((a.shape[0],), torch.float32)], pad_mode)[0]


def band_energy(waves, n_samples=None, pad_mode="constant"):
    """waves (B, n) f32 device rows -> (B, 1025) f32: E[b, f] = sum over the clip's own T(n_b) = 1 + n_b // 512 frames of |S_b[f, t]|
    at n_fft 2048, hop 512.  n_samples: int32 (B,) device tensor, clamped on the device to [1, n] ([1025, n] with
    pad_mode="reflect"); None: the rows are full."""
    w, ns = _one("band_energy", waves, n_samples, BAND_N_FFT, pad_mode)
    return _run("band_energy", (w,), (ns,), [((w.shape[0], BAND_BINS), torch.float32)], pad_mode)[0]


def instrumentation_similarity(a, b, n_a=None, n_b=None, pad_mode="constant"):
    """a (B, n), b (B, m) f32 device rows -> (B,) f32: Pearson's r of band_energy(a)[i] and band_energy(b)[i] over the 1025 bins,
    exactly 0.0 where r is not finite (a constant energy vector; the reference's nan -> 0.0).  The clips of a pair keep their own
    lengths."""
    for t, what in ((a, "a"), (b, "b")):
        _rows(t, "instrumentation_similarity", what, BAND_N_FFT, pad_mode)
    if a.shape[0] != b.shape[0]:
        raise ValueError(f"instrumentation_similarity: {a.shape[0]} and {b.shape[0]} rows")
    ea, eb = band_energy(a, n_a, pad_mode), band_energy(b, n_b, pad_mode)
    out = torch.empty(a.shape[0], dtype=torch.float32, device=ea.device)
    check(lib().ast_pearson_rows(ptr(ea), ptr(eb), a.shape[0], BAND_BINS, ptr(out), stream()), "ast_pearson_rows")
    return out


def _mfcc_args(name, n_mfcc, hop_length):
    if not isinstance(n_mfcc, int) or isinstance(n_mfcc, bool) or not 1 <= n_mfcc <= 128:
        raise ValueError(f"{name}: n_mfcc must be an integer in 1 .. 128, got {n_mfcc!r}")
    if hop_length not in MFCC_HOPS:
        raise ValueError(f"{name}: hop_length must be 256 or 512 (the reference's two values), got {hop_length!r}")


def mfcc(waves, n_samples=None, n_mfcc=20, hop_length=512, pad_mode="constant"):
    """waves (B, n) f32 device rows at 22 050 Hz -> (B, n_mfcc, T_max) f32, T_max = 1 + n // hop_length: what
    librosa.feature.mfcc(y, sr=22050, n_mfcc, hop_length) is documented to compute for clip b over its own n_b samples, in
    librosa's layout; frames t >= T_b = 1 + n_b // hop_length of clip b are exactly 0.  The chain: |STFT|^2 at n_fft 2048, Slaney
    mel filter bank (128 bands, 0 .. 11 025 Hz), 10 log10(max(1e-10, .)), clamped from below to the clip's own maximum - 80,
    orthonormal DCT-II along the bands.  n_samples: int32 (B,) device tensor, clamped on the device to [1, n] ([1025, n] with
    pad_mode="reflect"); None: the rows are full."""
    _mfcc_args("mfcc", n_mfcc, hop_length)
    w, ns = _one("mfcc", waves, n_samples, MFCC_N_FFT, pad_mode)
    B, n = w.shape
    return _run("mfcc", (w,), (ns,), [((B, n_mfcc, 1 + n // hop_length), torch.float32)], pad_mode, (n_mfcc, hop_length), (hop_length,), MFCC_SR)[0]


def mfcc_distance(generated, reference, n_generated=None, n_reference=None, n_mfcc=13, hop_length=256, pad_mode="constant"):
    """generated (B, n), reference (B, m) f32 device rows at 22 050 Hz -> (B,) f32: the mean over t < min(T_g, T_r) of
    ||mfcc(generated)[b, :, t] - mfcc(reference)[b, :, t]||_2 (evaluation_style_transfer.py:99-109; the defaults are its call).
    The clips of a pair keep their own lengths: nothing is truncated, each is clamped by its own maximum.  Equal clips score
    exactly 0."""
    _mfcc_args("mfcc_distance", n_mfcc, hop_length)
    g, r, ng, nr = _pair("mfcc_distance", generated, "generated", reference, "reference", n_generated, n_reference, MFCC_N_FFT, pad_mode)
    return _run("mfcc_distance", (g, r), (ng, nr), [((g.shape[0],), torch.float32)], pad_mode, (n_mfcc, hop_length), (hop_length,), MFCC_SR)[0]


# ---- chroma and pitch (csrc/chroma.hip): librosa.piptrack, estimate_tuning, filters.chroma and feature.chroma_stft restated as a
# formula chain ("Chroma and pitch"); parity with librosa's own output is unpinned
CHROMA_SETTINGS = ((2048, 512), (1024, 256))             # librosa's defaults (chroma_distance, pitch_correlation); chroma_similarity's call
N_CHROMA = 12


def _chroma_setting(name, n_fft, hop_length):
    if (n_fft, hop_length) not in CHROMA_SETTINGS:
        raise ValueError(f"{name}: (n_fft, hop_length) must be (2048, 512) or (1024, 256), the evaluation scripts' two settings, "
                         f"got ({n_fft!r}, {hop_length!r})")


def _tuning(w, ns, n_fft, hop_length, pad_mode, debug=None):
    B, n = w.shape
    L = lib()
    ws = torch.empty(L.ast_tuning_ws_floats(B, n, n_fft), dtype=torch.float32, device=w.device)
    out = torch.empty(B, dtype=torch.float32, device=w.device)
    check(L.ast_tuning_len(ptr(w), B, n, ptr(ns), None, n, n_fft, hop_length, PAD_MODES[pad_mode], ptr(ws), ws.numel(), ptr(out), ptr(debug),
                           stream()), "ast_tuning_len")
    return out


def estimate_tuning(waves, n_samples=None, n_fft=2048, hop_length=512, pad_mode="constant"):
    """waves (B, n) f32 device rows at 22 050 Hz -> (B,) f32: what librosa.estimate_tuning is documented to give as
    librosa.feature.chroma_stft calls it on clip b's own n_b samples -- piptrack's peaks of |STFT|^2 between 150 and 4000 Hz, those
    at or above the median magnitude, the fullest 0.01-semitone bin of their deviations from equal temperament; in [-0.5, 0.5),
    0.0 for a clip without a peak.  (n_fft, hop_length): (2048, 512) or (1024, 256).  n_samples: int32 (B,) device tensor, clamped
    on the device to [1, n] ([n_fft / 2 + 1, n] with pad_mode="reflect"); None: the rows are full."""
    _chroma_setting("estimate_tuning", n_fft, hop_length)
    return _tuning(*_one("estimate_tuning", waves, n_samples, n_fft, pad_mode), n_fft, hop_length, pad_mode)


def tuning_debug(waves, n_samples=None, n_fft=2048, hop_length=512, pad_mode="constant"):
    """estimate_tuning and what it counted -> (tuning (B,), candidates (B,) int32, kept (B,) int32, thr (B,) f32, histogram (B, 100) int32);
    for the tests"""
    _chroma_setting("tuning_debug", n_fft, hop_length)
    w, ns = _one("tuning_debug", waves, n_samples, n_fft, pad_mode)
    ptr(w)
    dbg = torch.zeros((w.shape[0], lib().ast_tuning_debug_words()), dtype=torch.int32, device=w.device)
    tuning = _tuning(w, ns, n_fft, hop_length, pad_mode, dbg)
    return tuning, dbg[:, 0], dbg[:, 1], dbg[:, 2].contiguous().view(torch.float32), dbg[:, 3:]


def chroma_stft(waves, n_samples=None, n_fft=2048, hop_length=512, pad_mode="constant", tuning=None):
    """waves (B, n) f32 device rows at 22 050 Hz -> (B, 12, T_max) f32, T_max = 1 + n // hop_length: what
    librosa.feature.chroma_stft(y, sr=22050, n_fft, hop_length) is documented to compute for clip b over its own n_b samples, in
    librosa's layout (row 0 = C, row 9 = A); frames t >= T_b are exactly 0.  The chain: |STFT|^2, librosa.filters.chroma's bank
    (Gaussians a semitone apart around the clip's tuning, unit L2 norm per bin, octave weighting around 5 octaves above 27.5 Hz),
    each frame divided by its maximum.  tuning: (B,) f32 device tensor in semitones, or None: estimate_tuning's.
    (n_fft, hop_length): (2048, 512) or (1024, 256).  n_samples as above."""
    _chroma_setting("chroma_stft", n_fft, hop_length)
    w, ns = _one("chroma_stft", waves, n_samples, n_fft, pad_mode)
    B, n = w.shape
    if tuning is None:
        tuning = _tuning(w, ns, n_fft, hop_length, pad_mode)
    elif not (torch.is_tensor(tuning) and tuning.dtype == torch.float32 and tuple(tuning.shape) == (B,)):
        raise ValueError(f"chroma_stft: tuning must be a float32 tensor of shape ({B},)")
    out = torch.empty((B, N_CHROMA, 1 + n // hop_length), dtype=torch.float32, device=w.device)
    check(lib().ast_chroma_len(ptr(w), B, n, ptr(ns), None, n, n_fft, hop_length, PAD_MODES[pad_mode], ptr(tuning.contiguous()), ptr(out),
                               stream()), "ast_chroma_len")
    return out


def chroma_distance(original, generated, n_original=None, n_generated=None, pad_mode="constant"):
    """original (B, n), generated (B, m) f32 device rows at 22 050 Hz -> (B,) f32: the mean over the frames of
    ||chroma_stft(original)[b, :, t] - chroma_stft(generated)[b, :, t]||_2 at n_fft 2048, hop 512 (evaluation_reconstruction.py:39-52),
    both clips cut to L_b = min(n_original[b], n_generated[b]) samples first (:193-204), each with its own tuning.  Equal clips score
    exactly 0."""
    a, g, na, ng = _pair("chroma_distance", original, "original", generated, "generated", n_original, n_generated, 2048, pad_mode)
    return _run("chroma_distance", (a, g), (na, ng), [((a.shape[0],), torch.float32)], pad_mode)[0]


def chroma_similarity(generated, original, n_generated=None, n_original=None, pad_mode="constant"):
    """generated (B, n), original (B, m) f32 device rows at 22 050 Hz -> (B,) f32: the mean over the 12 chroma rows of Pearson's r
    between chroma_stft(generated)[b, c] and chroma_stft(original)[b, c] at n_fft 1024, hop 256 over the frames t < min(T_g, T_o)
    (evaluation_style_transfer.py:80-96): the "content kept?" score.  The clips keep their own lengths; rows whose r is not finite
    are left out, and a pair without a finite row scores exactly 0.0."""
    g, a, ng, na = _pair("chroma_similarity", generated, "generated", original, "original", n_generated, n_original, 1024, pad_mode)
    return _run("chroma_similarity", (g, a), (ng, na), [((g.shape[0],), torch.float32)], pad_mode)[0]


def pitch_mean(waves, n_samples=None, pad_mode="constant"):
    """waves (B, n) f32 device rows at 22 050 Hz -> (B, T_max) f32, T_max = 1 + n // 512: np.mean(librosa.piptrack(y, sr)[0], axis=0)
    as documented, for clip b over its own n_b samples (n_fft 2048, hop 512; the interpolated peaks of |STFT| between 150 and
    4000 Hz above a tenth of the frame's maximum, averaged over all 1025 bins); frames t >= T_b are exactly 0."""
    w, ns = _one("pitch_mean", waves, n_samples, 2048, pad_mode)
    B, n = w.shape
    out = torch.empty((B, 1 + n // 512), dtype=torch.float32, device=w.device)
    check(lib().ast_pitch_mean_len(ptr(w), B, n, ptr(ns), None, n, PAD_MODES[pad_mode], ptr(out), stream()), "ast_pitch_mean_len")
    return out


def pitch_correlation(original, generated, n_original=None, n_generated=None, pad_mode="constant"):
    """original (B, n), generated (B, m) f32 device rows at 22 050 Hz -> (B,) f32: Pearson's r of the two clips' pitch_mean over
    the frames (evaluation_reconstruction.py:83-103), both clips cut to L_b = min(n_original[b], n_generated[b]) samples first
    (:193-204); exactly 0.0 where r is not finite or there are fewer than 2 frames."""
    a, g, na, ng = _pair("pitch_correlation", original, "original", generated, "generated", n_original, n_generated, 2048, pad_mode)
    return _run("pitch_correlation", (a, g), (na, ng), [((a.shape[0],), torch.float32)], pad_mode)[0]


# ---- onsets and self-similarity (csrc/metrics.hip): librosa.onset.onset_detect and librosa.segment.recurrence_matrix at their
# defaults restated as a formula chain ("Onsets and self-similarity"); parity with librosa's own output is unpinned
ONSET_HOP, SS_N_MFCC = 512, 20                            # librosa's default hop_length and n_mfcc


def _onset_one(name, waves, n_samples, pad_mode, out_dtype):
    w, ns = _one(name, waves, n_samples, MFCC_N_FFT, pad_mode)
    return _run(name, (w,), (ns,), [((w.shape[0], 1 + w.shape[1] // ONSET_HOP), out_dtype)], pad_mode, sample_rate=MFCC_SR)[0]


def onset_strength(waves, n_samples=None, pad_mode="constant"):
    """waves (B, n) f32 device rows at 22 050 Hz -> (B, T_max) f32, T_max = 1 + n // 512: the onset strength envelope that
    librosa.onset.onset_detect(y, sr=22050) is documented to build for clip b over its own n_b samples -- with dB the clamped mel rows
    of `mfcc` at hop 512, e[t] = the mean over the 128 bands of max(0, dB[m, t-2] - dB[m, t-3]) for 3 <= t < T_b; exactly 0 for t < 3
    and for t >= T_b = 1 + n_b // 512.  n_samples: int32 (B,) device tensor, clamped on the device to [1, n] ([1025, n] with
    pad_mode="reflect"); None: the rows are full."""
    return _onset_one("onset_strength", waves, n_samples, pad_mode, torch.float32)


def onset_detect(waves, n_samples=None, pad_mode="constant"):
    """waves (B, n) f32 device rows at 22 050 Hz -> (B, T_max) int32 mask: 1 where librosa.onset.onset_detect(y, sr=22050) at its
    defaults is documented to report frame t of clip b as an onset, 0 elsewhere and for t >= T_b.  A mask, not an index list: the
    shape does not depend on the data, so the call can be captured; `mask[b].nonzero()` gives librosa's frames.  No onsets where
    the envelope is all zero or not all finite; else the normalised envelope's peak picking with pre_max 1, post_max 1, pre_avg 4,
    post_avg 5, delta 0.07, wait 1 (0.03 sr // hop and so on at 22 050 Hz and hop 512).  n_samples as for onset_strength."""
    return _onset_one("onset_detect", waves, n_samples, pad_mode, torch.int32)


def onset_accuracy(original, generated, n_original=None, n_generated=None, pad_mode="constant"):
    """original (B, n), generated (B, m) f32 device rows at 22 050 Hz -> (B,) f32: the F1 score of the two clips' onset frames
    (evaluation_reconstruction.py:54-81), both clips cut to L_b = min(n_original[b], n_generated[b]) samples first (:193-204):
    1.0 if neither has an onset, 0.0 if exactly one has none, else 2 |O and G| / (|O| + |G|).  Equal clips score exactly 1."""
    a, g, na, ng = _pair("onset_accuracy", original, "original", generated, "generated", n_original, n_generated, MFCC_N_FFT, pad_mode)
    return _run("onset_accuracy", (a, g), (na, ng), [((a.shape[0],), torch.float32)], pad_mode, sample_rate=MFCC_SR)[0]


def _recurrence(name, waves, n_samples, pad_mode, debug):
    w, ns = _one(name, waves, n_samples, MFCC_N_FFT, pad_mode)
    shape = (w.shape[0], SS_N_MFCC, SS_N_MFCC)
    return tuple(_run("recurrence", (w,), (ns,), [(shape, torch.int32), (shape, torch.float32) if debug else None], pad_mode, sample_rate=MFCC_SR))


def recurrence_matrix(waves, n_samples=None, pad_mode="constant"):
    """waves (B, n) f32 device rows at 22 050 Hz -> (B, 20, 20) int32: what librosa.segment.recurrence_matrix(mfcc.T) at its defaults
    is documented to give for mfcc = librosa.feature.mfcc(y, sr=22050) of clip b over its own n_b samples
    (evaluation_style_transfer.py:122-126).  The reference hands over the transpose, so the matrix's points are the 20 coefficient
    rows, each a vector over the clip's T_b frames, and the result is 20 x 20 whatever the clip's length.  Orientation: R[b, i, j] = 1
    iff coefficient row i is one of the kept neighbours of row j -- of the 12 nearest other rows of j (ties to the lower index)
    those at distance exactly 0 are dropped and of the rest the 10 nearest are kept.  Column j holds at most 10 ones, the diagonal
    is 0, the matrix is not symmetrised.  A T x T matrix over time frames is not offered.  n_samples as for onset_strength."""
    return _recurrence("recurrence_matrix", waves, n_samples, pad_mode, False)[0]


def recurrence_debug(waves, n_samples=None, pad_mode="constant"):
    """recurrence_matrix and the squared distances it ranked -> (R (B, 20, 20) int32, dist2 (B, 20, 20) f32); for the tests"""
    return _recurrence("recurrence_debug", waves, n_samples, pad_mode, True)


def self_similarity_distance(a, b, n_a=None, n_b=None, pad_mode="constant"):
    """a (B, n), b (B, m) f32 device rows at 22 050 Hz -> (B,) f32: the mean over the 400 cells of
    |recurrence_matrix(a)[i] - recurrence_matrix(b)[i]| (evaluation_style_transfer.py:121-133), a multiple of 1 / 400.  Each clip is
    taken at its own length.  Equal clips score exactly 0."""
    a, b, na, nb = _pair("self_similarity_distance", a, "a", b, "b", n_a, n_b, MFCC_N_FFT, pad_mode)
    return _run("self_similarity_distance", (a, b), (na, nb), [((a.shape[0],), torch.float32)], pad_mode, sample_rate=MFCC_SR)[0]
