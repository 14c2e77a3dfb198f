#!/usr/bin/env python3
"""Times load_audio's resample + stereo mean for 8 stereo clips of mixed duration (section counts [2, 3, 4, 4, 5, 6, 8, 9] once at
22 050 Hz), and style transfer from those native-rate clips:

  operator, at 48 kHz (320 -> 147, the staged polyphase kernel) and at 44.1 kHz (2 -> 1, the staged halving):
    A  resample_batch   ast_resample_poly_len on the (8, 2, n_max) batch with the sample counts on the device
    B  rows + mean      the route there was before: ast_resample_poly on the (16, n_max) rows, then torch.mean over the pairs
                        (it filters the padding too and leaves the FIR's ringing behind every clip's end)
  session, bf16, 48 kHz:
    A  transfer         one replay of the graph of transfer(..., sample_rate=48000): resample, front end, models, reconstruction
    B  per clip         cqt.resample + torch.mean once per clip on the host side of the graph, pad_waveforms, one replay of
                        the existing transfer graph

Alternating A / B, 5 warm-up + 30 timed repetitions each.  The operator is timed with device events around the call, the session
with the host's wall clock around a synchronised call sequence (what a caller pays, input copies included); median and min..max.
Usage: python profiles/native_rate/bench_resample.py [out.txt]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-style-transfer_amd")]
import torch  # noqa: E402
import ast_amd  # noqa: E402
from ast_amd import config, cqt  # noqa: E402
from ast_amd import utilityFunctions as U  # noqa: E402
from ast_amd.infer import StyleTransferSession  # noqa: E402
from oracle import seeded_params as sp  # noqa: E402

N_SEC, REPS, WARM, DEV, NEW = [2, 3, 4, 4, 5, 6, 8, 9], 30, 5, "cuda", 22050


def model(tag, ctor):
    m = ctor()
    m.load_state_dict(sp.seeded_state_dict(m.state_dict(), tag=tag))
    return m.to(DEV).eval()


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternate(cands, clock):
    for _ in range(WARM):
        for fn in cands.values():
            fn()
    times = {k: [] for k in cands}
    for _ in range(REPS):
        for k, fn in cands.items():
            times[k].append(clock(fn))
    return [f"  {k:46s} median {statistics.median(t):8.4f}  min {min(t):8.4f}  max {max(t):8.4f}" for k, t in times.items()]


def native_clips(rate):
    """stereo clips at `rate` whose resampled lengths are the ragged benchmark's: k exactly filled sections plus a few samples"""
    n_22k = [256 * (191 * (k - 1) + 287 - 1) + 37 * b for b, k in enumerate(N_SEC)]
    n_in = [n * rate // NEW for n in n_22k]
    assert [cqt.resampled_length(n, rate, NEW) for n in n_in] == n_22k
    return [0.07 * sp.seeded_normal((2, n), 9300 + b).to(DEV) for b, n in enumerate(n_in)], n_in, n_22k


def main():
    lines = [f"resample + stereo mean of 8 stereo clips, section counts {N_SEC} at 22 050 Hz, {torch.cuda.get_device_name(0)}; "
             f"{WARM} warm-up + {REPS} timed repetitions, alternating; ms"]
    for rate in (48000, 44100):
        clips, n_in, n_22k = native_clips(rate)
        waves, n = U.pad_waveforms(clips, channels=2)
        rows = waves.reshape(16, -1)
        m = cqt.resampled_length(waves.shape[-1], rate, NEW)
        cands = {"A  resample_batch (8, 2, n) with lengths": lambda: cqt.resample_batch(waves, n, rate, NEW),
                 "B  ast_resample_poly on (16, n) rows + mean": lambda: cqt.resample(rows, rate, NEW).reshape(8, 2, m).mean(dim=1)}
        res = alternate(cands, event_ms)
        a, b = cands["A  resample_batch (8, 2, n) with lengths"]()[0], cands["B  ast_resample_poly on (16, n) rows + mean"]()
        same = all(bool(torch.equal(a[r, :k - 400], b[r, :k - 400])) for r, k in enumerate(n_22k))      # B rings near a clip's end
        lines += [f"operator at {rate} Hz: {sum(n_in) / rate:.1f} s of stereo audio, n_max = {waves.shape[-1]}, m = {m}; "
                  f"A equals B away from the clips' ends: {same}"] + res
    config.set_compute_dtype(torch.bfloat16)
    rate = 48000
    clips, n_in, n_22k = native_clips(rate)
    waves, n = U.pad_waveforms(clips, channels=2)
    cls = sp.seeded_normal((len(clips), 256), 9100).to(DEV)
    sess = StyleTransferSession(model("content", ast_amd.ContentEncoder), model("decoder", ast_amd.Decoder), use_graph=True)

    def per_clip():
        w, k = U.pad_waveforms([torch.mean(cqt.resample(c, rate, NEW), dim=0) for c in clips])
        return sess.transfer(w, cls, n_samples=k)

    cands = {"A  transfer(sample_rate=48000), one replay": lambda: sess.transfer(waves, cls, n_samples=n, sample_rate=rate),
             "B  resample + mean per clip, pad, one replay": per_clip}
    res = alternate(cands, wall_ms)
    a, b = cands["A  transfer(sample_rate=48000), one replay"](), per_clip()
    torch.cuda.synchronize()
    dev = float((a[0].double() - b[0].double()).abs().max() / b[0].double().abs().max())
    lines += [f"session, bf16, from 48 kHz stereo: graphs held {len(sess._graphs)}; A against B, waveforms: {dev:.2e} relative; "
              f"lengths equal: {bool(torch.equal(a[2], b[2]))}"] + res
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(text + "\n")


if __name__ == "__main__":
    main()
