"""Restatement of `librosa.stft`'s documented defaults and of the two evaluation metrics built on it (ast_amd/metrics.py), in a
dtype of the caller's choice: float64 is what the kernels are checked against, float32 on the CPU is the rounding floor of any
f32 implementation.  librosa itself is not used (parity with its output is unpinned, DESIGN 7 "Spectrogram metrics").

    frame t is centred on sample t * hop; T(n) = 1 + n // hop; periodic Hann window of n_fft;
    pad_mode "constant": samples outside [0, n) are 0; "reflect": reflected at the clip's own ends (no edge repeat).

Shared by tests/test_metrics_cpu.py and tests/test_gpu_metrics.py: the fixture clips, their counts and the references (computed
once per process)."""
import functools

import numpy as np
import torch

MSE_N_FFT, MSE_HOP = 1024, 256
BAND_N_FFT, BAND_HOP = 2048, 512

B, N_MAX = 4, 40000
COUNTS = {"constant": [40000, 1, 300, 20481], "reflect": [40000, 1025, 2049, 20481]}
N_GENERATED = [30000, 40000, 777, 20480]                 # the minimum of a pair comes from either side


def n_frames(n, hop):
    return 1 + n // hop


def magnitudes(x, n_fft, hop, pad_mode, dtype=torch.float64):
    """|STFT| of one clip (1-D, its own samples only) -> (n_fft // 2 + 1, T(n)), every step in `dtype`"""
    x = torch.as_tensor(x).to(dtype)
    n, half = x.numel(), n_fft // 2
    idx = torch.arange(-half, (n_frames(n, hop) - 1) * hop + half)
    if pad_mode == "reflect":
        assert n > half, "reflect padding needs more than n_fft / 2 samples"
        idx = idx.abs()
        idx = torch.where(idx >= n, 2 * (n - 1) - idx, idx)
        padded = x[idx]
    else:
        assert pad_mode == "constant"
        inside = (idx >= 0) & (idx < n)
        padded = torch.where(inside, x[idx.clamp(0, n - 1)], torch.zeros((), dtype=dtype))
    j = torch.arange(n_fft, dtype=torch.float64)
    window = (0.5 - 0.5 * torch.cos(2 * np.pi * j / n_fft)).to(dtype)                  # periodic Hann
    frames = padded.unfold(0, n_fft, hop) * window                                     # (T, n_fft)
    return torch.fft.rfft(frames, dim=1).abs().T


def mse_spectrogram(a, g, pad_mode="constant", dtype=torch.float64):
    """evaluation_reconstruction.py:193-204 (truncate the audio to the common length), then :105-118"""
    L = min(len(a), len(g))
    A, G = (magnitudes(x[:L], MSE_N_FFT, MSE_HOP, pad_mode, dtype) for x in (a, g))
    return ((A - G) ** 2).mean()


def band_energy(x, pad_mode="constant", dtype=torch.float64):
    """evaluation_style_transfer.py:112-115: sum of |S| over the frames -> (1025,)"""
    return magnitudes(x, BAND_N_FFT, BAND_HOP, pad_mode, dtype).sum(dim=1)


def pearson(ea, eb):
    """scipy.stats.pearsonr's r with the reference's nan -> 0.0 (evaluation_style_transfer.py:117-119)"""
    da, db = ea - ea.mean(), eb - eb.mean()
    r = (da * db).sum() / ((da * da).sum().sqrt() * (db * db).sum().sqrt())
    return r if bool(torch.isfinite(r)) else torch.zeros((), dtype=ea.dtype)


def instrumentation_similarity(a, b, pad_mode="constant", dtype=torch.float64):
    return pearson(band_energy(a, pad_mode, dtype), band_energy(b, pad_mode, dtype))


# ---- the fixture of the GPU tests -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture_waves():
    """(original, generated): two (B, N_MAX) batches of unit-normal samples, float32"""
    gen = torch.Generator().manual_seed(4100)
    return torch.randn(B, N_MAX, generator=gen), torch.randn(B, N_MAX, generator=gen)


def _rel(x, ref):
    return float((x.double() - ref).abs().max() / ref.abs().max())


@functools.lru_cache(maxsize=None)
def references(pad_mode, use_lengths=True):
    """float64 references of the fixture under `pad_mode` with its counts (use_lengths=False: every row taken as full):
    dict(mse (B,), energy (B, 1025) of `original`, energy_gen (B, 1025) of `generated` at N_GENERATED, sim (B,))"""
    a, g = fixture_waves()
    na, ng = (COUNTS[pad_mode], N_GENERATED) if use_lengths else ([N_MAX] * B, [N_MAX] * B)
    out = _evaluate(a, g, na, ng, pad_mode, torch.float64)
    return {k: v.double() for k, v in out.items()}


def _evaluate(a, g, na, ng, pad_mode, dtype):
    """each count clamped as the device clamps it: reflect padding needs more than n_fft / 2 samples"""
    lo = MSE_N_FFT // 2 + 1 if pad_mode == "reflect" else 1
    mse = torch.stack([mse_spectrogram(a[b, :max(na[b], lo)], g[b, :max(ng[b], lo)], pad_mode, dtype) for b in range(B)])
    lo = BAND_N_FFT // 2 + 1 if pad_mode == "reflect" else 1
    ea = torch.stack([band_energy(a[b, :max(na[b], lo)], pad_mode, dtype) for b in range(B)])
    eg = torch.stack([band_energy(g[b, :max(ng[b], lo)], pad_mode, dtype) for b in range(B)])
    sim = torch.stack([pearson(ea[b], eg[b]) for b in range(B)])
    return dict(mse=mse, energy=ea, energy_gen=eg, sim=sim)


def spread(e):
    """relative spread of an energy vector around its mean: 0 for a constant one, where Pearson's r is 0 / 0"""
    e = e.double()
    return float((e - e.mean()).norm() / e.norm()) if float(e.norm()) > 0 else 0.0


WELL_CONDITIONED = 1e-3        # rows whose two energy vectors both spread by more than this have an r that rounding cannot move much


@functools.lru_cache(maxsize=None)
def f32_floor(pad_mode):
    """The rounding floor: the same restatement evaluated in float32 on the CPU against its float64 form, on the fixture.
    mse: largest relative error over the rows; energy: largest error over a row's bins relative to the row's peak, over both
    batches; sim: largest absolute error over the rows whose r is well conditioned."""
    a, g = fixture_waves()
    na, ng = COUNTS[pad_mode], N_GENERATED
    ref, f32 = references(pad_mode), _evaluate(a, g, na, ng, pad_mode, torch.float32)
    ok = conditioned_rows(pad_mode)
    return dict(mse=max(abs(float(f32["mse"][b]) - float(ref["mse"][b])) / float(ref["mse"][b]) for b in range(B)),
                energy=max(_rel(f32[k][b], ref[k][b]) for k in ("energy", "energy_gen") for b in range(B)),
                sim=max(abs(float(f32["sim"][b]) - float(ref["sim"][b])) for b in ok))


def conditioned_rows(pad_mode):
    ref = references(pad_mode)
    return [b for b in range(B) if min(spread(ref["energy"][b]), spread(ref["energy_gen"][b])) > WELL_CONDITIONED]


def bounds(pad_mode):
    """10 x the float32 floor: the kernels' sincospif twiddles and the packed-FFT untangling add a few roundings over torch's tables"""
    return {k: 10 * v for k, v in f32_floor(pad_mode).items()}
