"""Drop-in for the torch-only part of the reference's utilityFunctions.py on libast_hip.

get_STFT runs the LDS-staged radix-4 FFT kernel; get_overlap_windows /
sections2spectrogram / concat_stft_cqt are index plumbing on device tensors.
inverse_STFT runs an inverse-FFT + overlap-add kernel pair.  get_CQT and load_audio live in cqt.py (librosa /
torchaudio arithmetic restated from their published algorithms: parity unpinned); inverse_CQT is not built.
"""
from __future__ import annotations

import torch

from ._lib import check, len_tensor, lib, ptr, stream
from .cqt import _len_call

WINDOW_SIZE = 287
OVERLAP_PERCENTAGE = 0.3
OVERLAP_FRAMES = 96


def _ident_stats(device):
    return torch.zeros(2, 513, device=device), torch.ones(2, 513, device=device) - 1e-8


def stft_sections(waves: torch.Tensor, mean=None, std=None, n_sections=None, F_total=513, out=None, n_samples=None):
    """waves (Bc, n) f32 cuda -> (Bc, S, 2, 287, F_total): STFT + z-score + windowing in one kernel
    (utilityFunctions.py:12-37,240-263; dataloader.py:9-13).  Bins >= 513 are left untouched.
    n_samples (int32 (Bc,) device tensor): the rows are zero-padded clips of n_samples[b] samples -- clip b is transformed as
    that clip alone (reflected at its own end), and its sections past its own count are 0 (ast_stft_sections_len)."""
    Bc, n = waves.shape
    T = 1 + n // 256
    step = WINDOW_SIZE - OVERLAP_FRAMES
    if n_sections is None:
        n_sections = len(section_starts(T))
    if mean is None:
        mean, std = _ident_stats(waves.device)
    if out is None:
        out = torch.zeros((Bc, n_sections, 2, WINDOW_SIZE, F_total), dtype=torch.float32, device=waves.device)
    _len_call("ast_stft_sections", (ptr(waves.contiguous()), Bc, n, ptr(mean.contiguous()), ptr(std.contiguous()), ptr(out), n_sections,
                                    WINDOW_SIZE, step, F_total),
              None if n_samples is None else (ptr(len_tensor(n_samples, Bc, "n_samples", contiguous=True)),))
    # version bump: the kernel wrote through the raw pointer (keeps version-keyed caches honest).  NOT `out.add_(0)`: that is a
    # read-modify-write of ALL bins on this stream, and the CQT kernel fills bins >= 513 of the same tensor on another stream
    # (train.Trainer._run_frontend) -- the no-op add wrote stale CQT bins back now and then (found by the mixed-length oracle test)
    torch.autograd.graph.increment_version(out)
    return out


def section_starts(n_time, window_size=WINDOW_SIZE, overlap_frames=OVERLAP_FRAMES):
    step, starts = window_size - overlap_frames, []
    for s in range(0, n_time, step):
        e = min(s + window_size, n_time)
        if e - s < window_size * 0.5:
            break
        starts.append(s)
        if e == n_time:
            break
    return starts


def get_STFT(waveform, n_fft=1024, hop_length=256):
    """utilityFunctions.py:12-37: (channels, samples) or (samples,) -> (2, T, 513)."""
    if n_fft != 1024 or hop_length != 256:
        raise NotImplementedError("the HIP front-end is built for n_fft=1024, hop=256 (the reference's only configuration)")
    w = waveform.reshape(1, -1).float()
    n = w.shape[1]
    T = 1 + n // 256
    # one "section" of T rows, step irrelevant: reuse the section kernel with win = T
    mean, std = _ident_stats(w.device)
    out = torch.empty((1, 1, 2, T, 513), dtype=torch.float32, device=w.device)
    check(lib().ast_stft_sections(ptr(w.contiguous()), 1, n, ptr(mean), ptr(std), ptr(out), 1, T, T, 513, stream()),
          "ast_stft_sections")
    return out[0, 0]


def get_overlap_windows(spectrogram, window_size=WINDOW_SIZE, overlap_frames=OVERLAP_FRAMES):
    """utilityFunctions.py:240-263: (2,T,F) -> (S,2,window,F); tails shorter than half a window are dropped."""
    Cc, n_time, n_freq = spectrogram.shape
    starts = section_starts(n_time, window_size, overlap_frames)
    out = spectrogram.new_zeros((len(starts), Cc, window_size, n_freq))
    for i, s in enumerate(starts):
        e = min(s + window_size, n_time)
        out[i, :, :e - s] = spectrogram[:, s:e]
    return out


def sections2spectrogram(sections, original_size, overlap=OVERLAP_FRAMES):
    """utilityFunctions.py:265-283: count-normalised overlap-average, (S,2,wind,F) -> (2,original_size,F), as one
    HIP kernel (ast_sections_overlap_avg)."""
    return sections2spectrogram_batch(sections.unsqueeze(0), original_size, overlap)[0]


def default_frames(n_sections, wind=WINDOW_SIZE, overlap=OVERLAP_FRAMES):
    """Frames that n sections cover, (wind - overlap) * (n - 1) + wind, elementwise on an int32 device tensor (no sync)."""
    return n_sections * (wind - overlap) + overlap


def pad_sections(clips):
    """Clips of different section counts, a list of (S_i, 2, 287, F) tensors on one device, as one zero-padded batch:
    -> (sections (B, S_max, 2, 287, F), n_sections int32 (B,)), both on that device."""
    if not clips:
        raise ValueError("pad_sections needs at least one clip")
    tail = tuple(clips[0].shape[1:])
    if any(c.dim() != 4 or tuple(c.shape[1:]) != tail or c.shape[0] < 1 for c in clips):
        raise ValueError(f"every clip must be (S_i >= 1, {', '.join(map(str, tail))}), got {[tuple(c.shape) for c in clips]}")
    n = [int(c.shape[0]) for c in clips]
    out = clips[0].new_zeros((len(clips), max(n)) + tail)
    for b, c in enumerate(clips):
        out[b, :n[b]] = c
    return out, torch.tensor(n, dtype=torch.int32, device=out.device)


def pad_waveforms(clips, channels=None):
    """Clips of different durations, a list of (n_i,) or (1, n_i) f32 tensors on one device, as one zero-padded batch:
    -> (waves (B, n_max), n_samples int32 (B,)), both on that device.
    channels = C (1 or 2): every clip is (C, n_i), as a decoder delivers it (stereo recordings for `transfer(..., sample_rate=)`)
    -> (waves (B, C, n_max), n_samples).  Without it a (2, n_i) clip is refused as before."""
    if not clips:
        raise ValueError("pad_waveforms needs at least one clip")
    if channels is not None:
        if channels not in (1, 2):
            raise ValueError(f"pad_waveforms: one or two channels expected, got {channels}")
        if any(not torch.is_tensor(c) or c.dim() != 2 or c.shape[0] != channels or c.shape[1] < 1 or c.dtype != torch.float32
               or c.device != clips[0].device for c in clips):
            raise ValueError(f"every clip must be a float32 ({channels}, n_i >= 1) tensor on one device, got "
                             f"{[(tuple(c.shape), c.dtype, str(c.device)) if torch.is_tensor(c) else type(c).__name__ for c in clips]}")
        n = [int(c.shape[1]) for c in clips]
        out = clips[0].new_zeros((len(clips), channels, max(n)))
        for b, c in enumerate(clips):
            out[b, :, :n[b]] = c
        return out, torch.tensor(n, dtype=torch.int32, device=out.device)
    flat = [c.reshape(-1) if torch.is_tensor(c) and (c.dim() == 1 or (c.dim() == 2 and c.shape[0] == 1)) else None for c in clips]
    if any(f is None or f.numel() < 1 or f.dtype != torch.float32 or f.device != flat[0].device for f in flat):
        raise ValueError("every clip must be a float32 (n_i >= 1,) or (1, n_i) tensor on one device, got "
                         f"{[(tuple(c.shape), c.dtype, str(c.device)) if torch.is_tensor(c) else type(c).__name__ for c in clips]}")
    n = [int(f.numel()) for f in flat]
    out = flat[0].new_zeros((len(flat), max(n)))
    for b, f in enumerate(flat):
        out[b, :n[b]] = f
    return out, torch.tensor(n, dtype=torch.int32, device=out.device)


def clip_lengths(ns, nsamp, window_size=WINDOW_SIZE, overlap_frames=OVERLAP_FRAMES):
    """Host twin of what the front-end kernels compute for a clip of `ns` samples in a row of `nsamp` (csrc/ast_lengths.h, the
    same function compiled for the host): (ns clamped to [NS_MIN, nsamp], frames T, sections, frames the sections cover)."""
    import ctypes
    out = (ctypes.c_int32 * 4)()
    check(lib().ast_frontend_lengths_host(int(ns), int(nsamp), window_size, window_size - overlap_frames, ctypes.byref(out)),
          "ast_frontend_lengths_host")
    return tuple(out)


def frontend_lengths(n_samples, nsamp):
    """n_samples int32 (B,) on the device -> (n_sections, n_frames) int32 (B,) on the device, no sync (ast_frontend_lengths)."""
    B = n_samples.shape[0]
    n_samples = len_tensor(n_samples, B, "n_samples", contiguous=True)
    n_sec, n_fr = torch.empty_like(n_samples), torch.empty_like(n_samples)
    check(lib().ast_frontend_lengths(ptr(n_samples), B, int(nsamp), WINDOW_SIZE, WINDOW_SIZE - OVERLAP_FRAMES, ptr(n_sec), ptr(n_fr), stream()),
          "ast_frontend_lengths")
    return n_sec, n_fr


def frontend_sections(waves, n_samples=None, stft_stats=None, cqt_stats=None):
    """The inference front end of process_audio (evaluation_style_transfer.py:135-146: get_STFT, get_CQT, normalize,
    concat_stft_cqt, get_overlap_windows) for a batch: waves (B, n_max) f32 on the device -> (x (B, S_max, 2, 287, 597),
    n_sections, n_frames), S_max = len(section_starts(1 + n_max // 256)).  stft_stats / cqt_stats: (mean, std) of (2, 513) /
    (2, 84), default none.  n_samples (int32 (B,) device tensor, e.g. from pad_waveforms): row b is a zero-padded clip of
    n_samples[b] samples and comes out as that clip alone, with 0 in its sections s >= n_sections[b]; the two int32 (B,)
    results stay on the device.  Without n_samples every clip is n_max long and both are None."""
    if waves.dim() != 2 or waves.dtype != torch.float32 or not waves.is_cuda:
        raise ValueError("frontend_sections: (B, n) float32 cuda waveforms expected")
    B, n = waves.shape
    S = len(section_starts(1 + n // 256))
    if S < 1:
        raise ValueError(f"frontend_sections: {n} samples give no section (at least {256 * ((WINDOW_SIZE + 1) // 2 - 1)} needed)")
    mean, std = stft_stats if stft_stats is not None else (None, None)
    x = torch.empty((B, S, 2, WINDOW_SIZE, 513 + 84), dtype=torch.float32, device=waves.device)
    cqt_sections(waves, x, *(cqt_stats if cqt_stats is not None else ()), n_samples=n_samples)
    stft_sections(waves, mean, std, n_sections=S, F_total=x.shape[-1], out=x, n_samples=n_samples)
    if n_samples is None:
        return x, None, None
    return (x,) + frontend_lengths(n_samples, n)


def sections2spectrogram_batch(sections, original_size, overlap=OVERLAP_FRAMES, n_bins=None, n_sections=None, n_frames=None):
    """Batched form: (B,S,2,wind,F) -> (B,2,original_size,n_bins or F).
    n_sections (int32 (B,) device tensor): a zero-padded batch -- clip b averages its sections k < n_sections[b] only, and its
    frames t >= n_frames[b] (int32 (B,); default: what its sections cover) come out as 0 (ast_sections_overlap_avg_len)."""
    B, S, _, wind, F = sections.shape
    hop = wind - overlap
    n_bins = F if n_bins is None else n_bins
    out_T = min(int(original_size), hop * (S - 1) + wind)
    sec = sections.float().contiguous()
    out = torch.empty((B, 2, out_T, n_bins), dtype=torch.float32, device=sec.device)
    if n_sections is None and n_frames is not None:
        raise ValueError("n_frames needs n_sections")
    tail = None
    if n_sections is not None:
        n_sections = len_tensor(n_sections, B, "n_sections", contiguous=True)
        n_frames = default_frames(n_sections, wind, overlap) if n_frames is None else len_tensor(n_frames, B, "n_frames", contiguous=True)
        tail = (ptr(n_sections), ptr(n_frames))
    _len_call("ast_sections_overlap_avg", (ptr(sec), ptr(out), B, S, wind, hop, F, n_bins, out_T), tail)
    return out


def concat_stft_cqt(stft, cqt):
    """utilityFunctions.py:285-299."""
    if stft.ndim != 3 or cqt.ndim != 3:
        raise ValueError(f"Both tensors must be 3D, got {stft.ndim}D e {cqt.ndim}D.")
    if stft.shape[0] != cqt.shape[0] or stft.shape[1] != cqt.shape[1]:
        raise ValueError(f"Channel/Time mismatch: stft {stft.shape[:2]} vs cqt {cqt.shape[:2]}")
    return torch.cat([stft, cqt], dim=2)


def inverse_STFT(stft_tensor, n_fft=1024, hop_length=256):
    """utilityFunctions.py:62-82: (2, T, 513) -> waveform (256*(T-1),) via the HIP inverse-FFT + overlap-add kernels."""
    if n_fft != 1024 or hop_length != 256:
        raise NotImplementedError("the HIP front-end is built for n_fft=1024, hop=256 (the reference's only configuration)")
    return inverse_STFT_batch(stft_tensor.unsqueeze(0))[0]


def inverse_STFT_batch(spec, n_frames=None):
    """(B, 2, T, 513) -> (B, 256*(T-1)) waveforms in one launch pair.
    n_frames (int32 (B,) device tensor): clip b is inverted as a clip of n_frames[b] frames (clamped to [2, T]); its samples
    from 256 * (n_frames[b] - 1) on are 0 (ast_istft_len)."""
    spec = spec.float().contiguous()
    B, _, T, _ = spec.shape
    frames = torch.empty((B, T, 1024), dtype=torch.float32, device=spec.device)
    wave = torch.empty((B, 256 * (T - 1)), dtype=torch.float32, device=spec.device)
    _len_call("ast_istft", (ptr(spec), B, T, ptr(frames), ptr(wave)),
              None if n_frames is None else (ptr(len_tensor(n_frames, B, "n_frames", contiguous=True)),))
    return wave


from .cqt import get_CQT, load_audio, resample, resample_batch, resampled_length, cqt_batch, cqt_sections  # noqa: E402,F401  (utilityFunctions.py:39-60,105-122)


def inverse_CQT(*a, **k):
    raise NotImplementedError("inverse_CQT (librosa.icqt, utilityFunctions.py:84-103) is off the train/inference path and not built")
