"""Dataset screening of the reference's Preprocessing_Dataset scripts on the device, for a padded batch of clips of different
lengths (csrc/curation.hip):

    frame_rms, silence_ratio   silent_tracks_dataset.py:20-27: librosa.feature.rms(y)[0] and the share of frames with rms < 0.005
    clip_rms, mfcc_mean        dataset_tracks_analysis.py:25-29: sqrt(mean(y^2)) and mean(librosa.feature.mfcc(y, sr, n_mfcc=13), axis=1);
                               dataset_variety.py:13-16: the same MFCC time-mean as a track's feature vector
    rms_normalize              unifies_violin_datasets.py:25-30: y * target / level, y itself where the level is 0
    sound_ratio                split_BachViolinDataset.py:24-30: is_mostly_sound, the share of 100 ms windows above -45 dBFS
    screen, DatasetReport      all of them in one call; the scripts' flagged list and summary lines

librosa's and pydub's documented definitions are restated, not linked, and parity with their own output is unpinned (DESIGN 7,
"Dataset screening").  The clips keep their own sample rate (the scripts load with sr=None): a rate enters only through the mel
table and the window length.  No length is read on the host, so every call can be captured in a graph; the mel table of a new
(device, sample_rate) is built on first use, which has to happen outside a capture."""
from __future__ import annotations

import torch

from ._lib import check, lib, ptr, stream
from .metrics import MFCC_HOPS, MFCC_N_FFT, PAD_MODES, _one, _run

RMS_FRAME, RMS_HOP = 2048, 512                           # librosa.feature.rms defaults: frame_length, hop_length
SILENCE_RMS, SILENCE_RATIO = 0.005, 0.3                  # rms_threshold, silence_ratio_threshold of silent_tracks_dataset.py
SOUND_MS, SOUND_DB, SOUND_RATIO = 100, -45.0, 0.6        # frame_size, silence_threshold, min_sound_ratio of split_BachViolinDataset.py
TARGET_RMS = 0.07                                        # target_rms of unifies_violin_datasets.py
MAX_N_MFCC = 20


def _frame_rms(name, waves, n_samples, threshold, pad_mode):
    """-> dict(rms (B, T_max), n_frames, silent (B,) int32, silence_ratio, level (B,) f32, sumsq (B,) f64, w, ns)"""
    w, ns = _one(name, waves, n_samples, RMS_FRAME, pad_mode)
    B, n = w.shape
    L = lib()
    ptr(w)
    dev = w.device
    ws = torch.empty((L.ast_frame_rms_ws_floats(B, n) + 1) // 2, dtype=torch.float64, device=dev)      # doubles: 8-byte aligned
    out = dict(rms=torch.empty((B, 1 + n // RMS_HOP), dtype=torch.float32, device=dev),
               n_frames=torch.empty(B, dtype=torch.int32, device=dev), silent=torch.empty(B, dtype=torch.int32, device=dev),
               silence_ratio=torch.empty(B, dtype=torch.float32, device=dev), level=torch.empty(B, dtype=torch.float32, device=dev),
               sumsq=torch.empty(B, dtype=torch.float64, device=dev))
    check(L.ast_frame_rms_len(ptr(w), B, n, ptr(ns), float(threshold), PAD_MODES[pad_mode], ptr(ws), 2 * ws.numel(), ptr(out["rms"]),
                              ptr(out["n_frames"]), ptr(out["silent"]), ptr(out["silence_ratio"]), ptr(out["level"]), ptr(out["sumsq"]),
                              stream()), "ast_frame_rms_len")
    out["w"], out["ns"] = w, ns
    return out


def frame_rms(waves, n_samples=None, pad_mode="constant"):
    """waves (B, n) f32 device rows -> (B, T_max) f32, T_max = 1 + n // 512: what librosa.feature.rms(y)[0] at its defaults
    (frame_length 2048, hop_length 512, centred) is documented to give for clip b over its own n_b samples -- rms[b, t] = the root of
    the mean of the padded clip's 2048 samples [512 t - 1024, 512 t + 1024) squared; frames t >= T_b = 1 + n_b // 512 are exactly 0.
    n_samples: int32 (B,) device tensor, clamped on the device to [1, n] ([1025, n] with pad_mode="reflect"); None: the rows are full."""
    return _frame_rms("frame_rms", waves, n_samples, SILENCE_RMS, pad_mode)["rms"]


def silence_ratio(waves, n_samples=None, threshold=SILENCE_RMS, pad_mode="constant"):
    """waves (B, n) f32 device rows -> (B,) f32: the share of clip b's T_b frames with frame_rms < threshold
    (silent_tracks_dataset.py:23-24; the script flags a track at >= 0.3)."""
    return _frame_rms("silence_ratio", waves, n_samples, threshold, pad_mode)["silence_ratio"]


def clip_rms(waves, n_samples=None):
    """waves (B, n) f32 device rows -> (B,) f32: sqrt(mean(y ** 2)) over clip b's own n_b samples (dataset_tracks_analysis.py:27),
    summed in a fixed order in double and rounded once."""
    return _frame_rms("clip_rms", waves, n_samples, SILENCE_RMS, "constant")["level"]


def _window(name, sample_rate, frame_ms):
    for v, what in ((sample_rate, "sample_rate"), (frame_ms, "frame_ms")):
        if not isinstance(v, int) or isinstance(v, bool) or v < 1:
            raise ValueError(f"{name}: {what} must be a positive integer, got {v!r}")
    win = sample_rate * frame_ms // 1000
    if win < 1:
        raise ValueError(f"{name}: a window of {frame_ms} ms holds no sample at {sample_rate} Hz")
    return win


def _sound(name, w, ns, sample_rate, frame_ms, threshold_db):
    """-> (mask (B, W_max) int32, ratio (B,) f32)"""
    win = _window(name, sample_rate, frame_ms)
    B, n = w.shape
    ptr(w)
    mask = torch.empty((B, n // win), dtype=torch.int32, device=w.device)
    ratio = torch.empty(B, dtype=torch.float32, device=w.device)
    check(lib().ast_window_sound_len(ptr(w), B, n, ptr(ns), win, float(threshold_db), ptr(mask) if mask.numel() else None, ptr(ratio),
                                     stream()), "ast_window_sound_len")
    return mask, ratio


def sound_windows(waves, n_samples=None, sample_rate=22050, frame_ms=SOUND_MS, threshold_db=SOUND_DB):
    """waves (B, n) f32 device rows -> (B, W_max) int32 mask, W_max = n // win, win = sample_rate * frame_ms // 1000: 1 where window w
    of clip b (its samples [w win, (w + 1) win)) has 20 log10(rms) > threshold_db at full scale 1.0, 0 elsewhere and for
    w >= W_b = n_b // win.  A window whose rms is 0 is never sound."""
    return _sound("sound_windows", *_one("sound_windows", waves, n_samples, RMS_FRAME, "constant"), sample_rate, frame_ms, threshold_db)[0]


def sound_ratio(waves, n_samples=None, sample_rate=22050, frame_ms=SOUND_MS, threshold_db=SOUND_DB):
    """waves (B, n) f32 device rows -> (B,) f32: the share of clip b's W_b windows that sound_windows marks, exactly 0.0 when the clip
    is shorter than a window (is_mostly_sound, split_BachViolinDataset.py:24-30; the script keeps a clip at >= 0.6).  pydub computes
    the level on int16 samples with an integer RMS; this is the same rule on float samples."""
    return _sound("sound_ratio", *_one("sound_ratio", waves, n_samples, RMS_FRAME, "constant"), sample_rate, frame_ms, threshold_db)[1]


def _mfcc_mean_args(name, sample_rate, n_mfcc, hop_length):
    if not isinstance(sample_rate, int) or isinstance(sample_rate, bool) or sample_rate < 1:
        raise ValueError(f"{name}: sample_rate must be a positive integer, got {sample_rate!r}")
    if not isinstance(n_mfcc, int) or isinstance(n_mfcc, bool) or not 1 <= n_mfcc <= MAX_N_MFCC:
        raise ValueError(f"{name}: n_mfcc must be an integer in 1 .. {MAX_N_MFCC}, got {n_mfcc!r}")
    if hop_length not in MFCC_HOPS:
        raise ValueError(f"{name}: hop_length must be 256 or 512, got {hop_length!r}")


def _mfcc_mean(w, ns, sample_rate, n_mfcc, hop_length, pad_mode):
    return _run("mfcc_mean", (w,), (ns,), [((w.shape[0], n_mfcc), torch.float32)], pad_mode, (n_mfcc, hop_length), (hop_length,), sample_rate)[0]


def mfcc_mean(waves, n_samples=None, sample_rate=22050, n_mfcc=13, hop_length=512, pad_mode="constant"):
    """waves (B, n) f32 device rows at `sample_rate` -> (B, n_mfcc) f32: np.mean(librosa.feature.mfcc(y, sr, n_mfcc), axis=1) as
    documented, for clip b over its own n_b samples (dataset_tracks_analysis.py:28-29, dataset_variety.py:13-16).  The DCT is linear,
    so this is the DCT (in double) of the time-mean of the clip's clamped mel dB rows; the per-frame coefficients never exist.
    n_mfcc <= 20.  n_samples as for frame_rms."""
    _mfcc_mean_args("mfcc_mean", sample_rate, n_mfcc, hop_length)
    return _mfcc_mean(*_one("mfcc_mean", waves, n_samples, MFCC_N_FFT, pad_mode), sample_rate, n_mfcc, hop_length, pad_mode)


def _target(name, target_rms):
    if isinstance(target_rms, bool) or not isinstance(target_rms, (int, float)) or not 0 < target_rms < float("inf"):
        raise ValueError(f"{name}: target_rms must be a positive finite number, got {target_rms!r}")
    return float(target_rms)


def rms_normalize(waves, n_samples=None, target_rms=TARGET_RMS, out=None):
    """waves (B, n) f32 device rows -> a tensor like waves: clip b scaled to the level target_rms over its own n_b samples, exactly 0
    behind them (rms_normalize, unifies_violin_datasets.py:25-30).  The gain target_rms / level is formed in double from clip_rms's
    sum and rounded once; a clip whose level is 0 is returned unchanged.  out: None, or a contiguous tensor like waves to write to,
    which may be waves itself."""
    target = _target("rms_normalize", target_rms)
    r = _frame_rms("rms_normalize", waves, n_samples, SILENCE_RMS, "constant")
    w, ns = r["w"], r["ns"]
    if out is None:
        out = torch.empty_like(w)
    elif not (torch.is_tensor(out) and out.dtype == torch.float32 and out.shape == w.shape and out.is_contiguous() and out.device == w.device):
        raise ValueError("rms_normalize: out must be a contiguous float32 tensor like waves on the same device")
    check(lib().ast_gain_rows_len(ptr(w), w.shape[0], w.shape[1], ptr(ns), ptr(r["sumsq"]), target, ptr(out), stream()), "ast_gain_rows_len")
    return out


def screen(waves, n_samples=None, sample_rate=22050, n_mfcc=13, hop_length=512, silence_threshold=SILENCE_RMS, frame_ms=SOUND_MS,
           threshold_db=SOUND_DB, pad_mode="constant"):
    """Everything the screening scripts ask of a clip, in one call -> dict of device tensors:
        rms_level (B,) f32       clip_rms
        silence_ratio (B,) f32   silence_ratio at silence_threshold
        sound_ratio (B,) f32     sound_ratio at frame_ms, threshold_db
        mfcc_mean (B, n_mfcc)    mfcc_mean at sample_rate, hop_length
        n_frames (B,) int32      T_b = 1 + n_b // 512, the frames silence_ratio counted over
    each bit-identical to the single call.  waves: (B, n) f32 device rows, or (B, C, n) with C <= 2 channels, which are averaged first
    (librosa.load's mono).  One pass over the samples for the levels, one for the windows, one mel pass; no length is read on the host,
    so the call can be captured in a graph once the mel table of (device, sample_rate) exists (any earlier call builds it)."""
    _mfcc_mean_args("screen", sample_rate, n_mfcc, hop_length)
    _window("screen", sample_rate, frame_ms)
    if torch.is_tensor(waves) and waves.dim() == 3:
        if not 1 <= waves.shape[1] <= 2 or waves.dtype != torch.float32:
            raise ValueError(f"screen: waves must be (B, n) or (B, C <= 2, n) float32 rows, got {waves.dtype} {tuple(waves.shape)}")
        waves = waves[:, 0] if waves.shape[1] == 1 else (waves[:, 0] + waves[:, 1]) * 0.5
    r = _frame_rms("screen", waves, n_samples, silence_threshold, pad_mode)
    w, ns = r["w"], r["ns"]
    level = r["level"] if pad_mode == "constant" else _frame_rms("screen", w, ns, silence_threshold, "constant")["level"]
    return dict(rms_level=level, silence_ratio=r["silence_ratio"], sound_ratio=_sound("screen", w, ns, sample_rate, frame_ms, threshold_db)[1],
                mfcc_mean=_mfcc_mean(w, ns, sample_rate, n_mfcc, hop_length, pad_mode), n_frames=r["n_frames"])


class DatasetReport:
    """Host accumulator of `screen` results and file names: the flagged list of silent_tracks_dataset.py:26-27 and the lines of
    summarize_statistics (dataset_tracks_analysis.py:48-54).

        report = DatasetReport()
        report.add(names, ast_amd.screen(waves, n_samples, sample_rate=sr), n_samples, sr)    # once per batch
        report.flagged()                    # [(filename, silence_ratio)] with silence_ratio >= 0.3, sorted by name
        print(report.summary("Dataset 1"))

    add() copies the batch's results to the host (one synchronisation per batch)."""

    def __init__(self, silence_ratio_threshold=SILENCE_RATIO):
        self.silence_ratio_threshold = float(silence_ratio_threshold)
        self.stats = dict(filenames=[], durations=[], rms_levels=[], sample_rates=[], mfcc_means=[], silence_ratios=[], sound_ratios=[])

    def add(self, filenames, result, n_samples, sample_rate):
        """filenames: B names; result: screen's dict; n_samples: the clips' sample counts (tensor or list); sample_rate: int, or B ints"""
        names = list(filenames)
        B = len(names)
        counts = [int(v) for v in (n_samples.tolist() if torch.is_tensor(n_samples) else n_samples)]
        rates = [int(sample_rate)] * B if isinstance(sample_rate, int) else [int(v) for v in sample_rate]
        host = {k: result[k].detach().cpu() for k in ("rms_level", "silence_ratio", "sound_ratio", "mfcc_mean")}
        if not (len(counts) == len(rates) == B and all(tuple(host[k].shape[:1]) == (B,) for k in host)):
            raise ValueError(f"DatasetReport.add: {B} names for {len(counts)} counts, {len(rates)} rates and {host['rms_level'].shape[0]} results")
        s = self.stats
        s["filenames"] += names
        s["durations"] += [c / r for c, r in zip(counts, rates)]                       # librosa.get_duration(y=y, sr=sr)
        s["rms_levels"] += host["rms_level"].double().tolist()
        s["sample_rates"] += rates
        s["mfcc_means"] += [row.double().tolist() for row in host["mfcc_mean"]]
        s["silence_ratios"] += host["silence_ratio"].double().tolist()
        s["sound_ratios"] += host["sound_ratio"].double().tolist()

    def flagged(self):
        """[(filename, silence_ratio)] of the tracks with silence_ratio >= the threshold, in sorted file order"""
        s = self.stats
        return [(f, r) for f, r in sorted(zip(s["filenames"], s["silence_ratios"])) if r >= self.silence_ratio_threshold]

    def mostly_sound(self, min_sound_ratio=SOUND_RATIO):
        """{filename: is_mostly_sound} (split_BachViolinDataset.py:30)"""
        return {f: r >= min_sound_ratio for f, r in zip(self.stats["filenames"], self.stats["sound_ratios"])}

    def summary(self, name):
        """the text summarize_statistics(name, stats) prints"""
        s = self.stats
        n = len(s["filenames"])
        if n == 0:
            raise ValueError("DatasetReport.summary: nothing was added")
        mean = lambda v: sum(v) / len(v)                                               # noqa: E731
        return "\n".join([f"\n{name}",
                          f"• Files analyzed: {n}",
                          f"• Average duration: {mean(s['durations']):.2f} sec",
                          f"• Average RMS: {mean(s['rms_levels']):.4f}",
                          f"• Unique sample rates: {set(s['sample_rates'])}",
                          f"• Global average MFCC (first coefficient).: {mean([m[0] for m in s['mfcc_means']]):.2f}"])
