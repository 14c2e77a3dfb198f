"""Inference pipeline of the reference's `process_audio` (evaluation_style_transfer.py:135-159) on the HIP path:

    sections (B,S,2,287,597) -> ContentEncoder -> Decoder (autoregressive, new_decoder.py:272-319, target_length=S)
             -> sections2spectrogram (overlap-average) -> inverse_STFT -> waveforms (B, 256*(T-1))

for a batch of clips, replayed as ONE hipGraph per input shape (the eager form is ~300 small launches per batch and
launch-bound).  Class embeddings are an input, as in the reference (a per-class table built beforehand).

Clips of different lengths go through one graph too: pad them to the longest (utilityFunctions.pad_sections) and pass
`n_sections`.  The per-clip counts stay on the device and are read by the kernels, so one graph per (B, S_max) serves
every mix of lengths ("Ragged inference batches").

From waveforms, as `process_audio` starts: `waves, n = utilityFunctions.pad_waveforms(clips)`, then
`session.transfer(waves, class_emb, n_samples=n)` runs front end, models and reconstruction as one graph per (B, n_max); the
per-clip sample counts stay on the device as well ("Ragged waveforms").  Recordings as they are decoded, at 44.1 or
48 kHz and stereo: `waves, n = utilityFunctions.pad_waveforms(clips, channels=2)`, then
`session.transfer(waves, class_emb, n_samples=n, sample_rate=48000)`; the resample and the channel mean run inside the same graph
("Native-rate, stereo recordings")."""
from __future__ import annotations

import torch

from . import config
from . import utilityFunctions as U
from ._lib import len_tensor

SAMPLE_RATE = 22050                                      # the models' rate: what load_audio resamples to


def replay_graph(graphs, use_graph, key, fn, inputs):
    """fn(*inputs), as one hipGraph per key of the cache `graphs`: captured on first use over clones of the inputs (after two
    warm-up runs on a side stream: weight banks -- eval: sigma from the stored u, v -- and caches), then replayed, with every input
    that is not its clone already copied in first.  Returns the captured outputs.  Without use_graph: fn(*inputs).  fn must leave
    no state behind (an eval-mode, no-grad pass): the warm-up runs are real runs.  The inference session and Trainer.evaluate
    replay through here."""
    if not use_graph:
        return fn(*inputs)
    if key not in graphs:
        static = [t.detach().clone() for t in inputs]
        side = torch.cuda.Stream(device=inputs[0].device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                fn(*static)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            outs = fn(*static)
        graphs[key] = (g, static, outs)
    g, static, outs = graphs[key]
    for dst, src in zip(static, inputs):
        if dst.data_ptr() != src.data_ptr():
            dst.copy_(src)
    g.replay()
    return outs


class StyleTransferSession:
    def __init__(self, content_encoder, decoder, use_graph: bool = True, overlap: int = U.OVERLAP_FRAMES):
        self.content, self.decoder = content_encoder.eval(), decoder.eval()
        self.use_graph, self.overlap = use_graph, overlap
        self._graphs = {}

    def _run(self, sections, class_emb, frames, n_sections=None, n_frames=None):
        """frames: the batch's frame count (int, from S_max).  n_sections, n_frames: int32 (B,) on the device for a padded batch
        (-> waveforms, stft sections, lengths), or both None for equal clips (-> waveforms, stft sections)."""
        with torch.no_grad():
            if n_sections is None:
                content_emb = self.content(sections)
                out = self.decoder(content_emb, class_emb, target_length=content_emb.size(1))   # (B,S,2,287,513)
                spec = U.sections2spectrogram_batch(out, frames, self.overlap)
                return U.inverse_STFT_batch(spec), out
            content_emb = self.content(sections, n_sections)
            out = self.decoder(content_emb, class_emb, target_length=content_emb.size(1), lengths=n_sections)
            nf = n_frames.clamp(2, frames)              # what the two kernels clamp to, so `lengths` says what they wrote
            spec = U.sections2spectrogram_batch(out, frames, self.overlap, n_sections=n_sections, n_frames=nf)
            return U.inverse_STFT_batch(spec, nf), out, (nf - 1) * 256

    def _replay(self, key, fn, inputs):
        return replay_graph(self._graphs, self.use_graph, key, fn, inputs)

    def __call__(self, sections: torch.Tensor, class_emb: torch.Tensor, original_frames=None, n_sections: torch.Tensor = None):
        """sections (B,S,2,287,597) f32, class_emb (B,d) f32 on the device -> (waveforms (B, 256*(T-1)), stft sections).

        n_sections (int32 (B,) device tensor): the batch is zero-padded to S sections and clip b holds n_sections[b] of them.
        original_frames may then be an int32 (B,) device tensor as well (default per clip: the frames its sections cover,
        191 * (n_b - 1) + 287, formed on the device).  Returns (waveforms, stft sections, lengths): lengths[b] =
        256 * (frames_b - 1) samples of waveforms[b] are clip b, the rest of the row is 0; output sections s >= n_b are
        finite and unspecified (exactly 0 with SimpleDecoder_TransformerOnly.Decoder).  No length is read on the host:
        every mix of lengths at one (B, S) replays the same graph."""
        B, S, _, wind, _ = sections.shape
        if n_sections is not None:
            return self._call_ragged(sections, class_emb, original_frames, n_sections)
        frames = original_frames or (wind - self.overlap) * (S - 1) + wind
        key = (tuple(sections.shape), tuple(class_emb.shape), frames, config.compute_dtype)
        return self._replay(key, lambda sec, cls: self._run(sec, cls, frames), [sections, class_emb])

    def _call_ragged(self, sections, class_emb, original_frames, n_sections):
        B, S, _, wind, _ = sections.shape
        frames = (wind - self.overlap) * (S - 1) + wind
        for name, t in (("n_sections", n_sections), ("original_frames", original_frames)):
            len_tensor(t, B, f"with n_sections, {name}", device=True)
        n_frames = U.default_frames(n_sections, wind, self.overlap) if original_frames is None else original_frames
        key = (tuple(sections.shape), tuple(class_emb.shape), frames, config.compute_dtype, "ragged")
        return self._replay(key, lambda sec, cls, n, f: self._run(sec, cls, frames, n, f), [sections, class_emb, n_sections, n_frames])

    def _run_wave(self, waves, class_emb, n_samples, frames, stft_stats, cqt_stats, sample_rate=None):
        if sample_rate is not None:                                  # native-rate and / or stereo rows: load_audio's resample + mean
            waves, n_samples = U.resample_batch(waves, n_samples, sample_rate, SAMPLE_RATE)
        x, n_sections, n_frames = U.frontend_sections(waves, n_samples, stft_stats, cqt_stats)
        return self._run(x, class_emb, frames, n_sections, n_frames)

    def _transfer_plan(self, waves, class_emb, n_samples, stft_stats, cqt_stats, sample_rate):
        """transfer's argument checks -> (graph key, inputs, frames, native rate or None, number of STFT statistics tensors)"""
        if not torch.is_tensor(waves) or waves.dim() not in (2, 3) or waves.dtype != torch.float32:
            raise ValueError("transfer: (B, n) or (B, C, n) float32 cuda waveforms expected")
        if int(sample_rate) != sample_rate or sample_rate <= 0:
            raise ValueError(f"transfer: sample_rate must be a positive integer, got {sample_rate}")
        B, n = waves.shape[0], waves.shape[-1]
        native = None if (sample_rate == SAMPLE_RATE and waves.dim() == 2) else int(sample_rate)
        if native is not None:
            C = waves.shape[1] if waves.dim() == 3 else 1
            if C not in (1, 2):
                raise ValueError(f"transfer: one or two channels expected, got {C}")
            n = U.resampled_length(n, native, SAMPLE_RATE)
            ns_min = max(513, 256 * ((U.WINDOW_SIZE + 1) // 2 - 1))
            if n < ns_min:
                raise ValueError(f"transfer: {waves.shape[-1]} samples at {native} Hz give {n} at {SAMPLE_RATE} Hz, the front end needs "
                                 f"{ns_min}")
        if not waves.is_cuda:
            raise ValueError("transfer: (B, n) or (B, C, n) float32 cuda waveforms expected")
        if n_samples is None:                                        # every clip fills its row (counted at the rate of `waves`)
            n_samples = torch.full((B,), waves.shape[-1], dtype=torch.int32, device=waves.device)
        len_tensor(n_samples, B, "n_samples", device=True)
        if len(U.section_starts(1 + n // 256)) < 1:
            raise ValueError(f"transfer: {n} samples give no section")
        frames = U.clip_lengths(n, n, U.WINDOW_SIZE, self.overlap)[3]
        stats = [t for pair in (stft_stats, cqt_stats) if pair is not None for t in pair]
        k = 2 if stft_stats is not None else 0

        key = (tuple(waves.shape), tuple(class_emb.shape), frames, config.compute_dtype, "ragged", "waves",
               stft_stats is not None, cqt_stats is not None)
        if native is not None:
            key += (native, C)
        return key, [waves, class_emb, n_samples] + stats, frames, native, k

    def transfer(self, waves: torch.Tensor, class_emb: torch.Tensor, n_samples: torch.Tensor = None, stft_stats=None, cqt_stats=None,
                 sample_rate: int = SAMPLE_RATE):
        """Waveform in, waveform out (evaluation_style_transfer.py:135-159 for a batch): waves (B, n_max) f32 and class_emb
        (B, d) f32 on the device -> (waveforms (B, 256 * (frames - 1)), stft sections (B, S_max, 2, 287, 513), lengths).

        n_samples (int32 (B,) device tensor, e.g. from utilityFunctions.pad_waveforms): row b of waves is a zero-padded clip of
        n_samples[b] samples, clamped on the device to [36 608, n_max].  Clip b has T_b = 1 + n_b // 256 frames, the sections
        the reference cuts from them, and comes back as lengths[b] = 256 * (frames_b - 1) samples, frames_b = min(T_b, what
        its sections cover); the rest of its row is 0.  `frames` above is that count for a clip of n_max samples.  Without
        n_samples every clip is n_max long (the same path, the counts filled in on the device).  stft_stats / cqt_stats:
        (mean, std) of the z-score, (2, 513) / (2, 84), default none.  No length is read on the host: every mix of durations
        at one (B, n_max) replays the same graph.

        sample_rate: the rate of `waves`, which may then be (B, C, n_max) with C <= 2 channels (a recording as it is decoded:
        evaluation_style_transfer.py:162-171, load_audio).  n_samples counts samples at that rate.  Anything but (B, n) rows at
        22 050 Hz goes through cqt.resample_batch first, inside the graph: clip b becomes the ceil(n_b * 22050 / sample_rate)
        samples that `resample` and the mean over its channels give it alone, and everything above holds for those; the outputs
        are at 22 050 Hz."""
        key, inputs, frames, native, k = self._transfer_plan(waves, class_emb, n_samples, stft_stats, cqt_stats, sample_rate)

        def run(wav, cls, n, *st):                                   # st: the (mean, std) pairs that were given, flattened as `stats`
            return self._run_wave(wav, cls, n, frames, st[:k] or None, st[k:] or None, native)

        return self._replay(key, run, inputs)

    def transfer_and_score(self, waves: torch.Tensor, class_emb: torch.Tensor, n_samples: torch.Tensor = None, reference: torch.Tensor = None,
                           n_reference: torch.Tensor = None, mfcc: bool = False, chroma: bool = False, onsets: bool = False,
                           self_similarity: bool = False, **transfer_kw):
        """`transfer` and the spectrogram metrics of its output (ast_amd.metrics) as one graph under a key of its own
        -> (waveforms, stft sections, lengths, scores); the first three are what `transfer` returns for the same arguments
        (transfer_kw: stft_stats, cqt_stats, sample_rate).

        scores["mse_spectrogram"] (B,): the output against the input at 22 050 Hz, clip b over min(its input count -- after
        resample_batch, the device-side n_out, when sample_rate is given --, lengths[b]) samples
        (evaluation_reconstruction.py:193-204, 105-118).
        reference (B, m) f32 device rows at 22 050 Hz, n_reference int32 (B,) device tensor or None for full rows:
        scores["instrumentation_similarity"] (B,) scores the output, over lengths[b] samples, against it
        (evaluation_style_transfer.py:111-119).
        mfcc=True (needs a reference): scores["mfcc_distance"] (B,) as well, the output over lengths[b] samples against the
        reference over n_reference[b], at 13 coefficients and hop 256 (evaluation_style_transfer.py:99-109), in the same graph,
        which then has a key of its own; the default leaves the call as it was.
        chroma=True (needs no reference): scores["chroma_similarity"] (B,) as well, the output over lengths[b] samples against the
        input at 22 050 Hz over its own count, at n_fft 1024, hop 256 (evaluation_style_transfer.py:80-96), in the same graph,
        again under a key of its own.
        onsets=True (needs no reference): scores["onset_accuracy"] (B,) as well, the output against the input under the length rule of
        scores["mse_spectrogram"] (evaluation_reconstruction.py:54-81).
        self_similarity=True (needs a reference): scores["self_similarity_distance"] (B,) as well, the output over lengths[b] samples
        against the reference over n_reference[b] (evaluation_style_transfer.py:121-133).  Each flag adds its own word to the key.
        All with pad_mode="constant".  No length is read on the host."""
        from . import metrics as M
        key, inputs, frames, native, k = self._transfer_plan(waves, class_emb, n_samples, transfer_kw.pop("stft_stats", None),
                                                             transfer_kw.pop("cqt_stats", None), transfer_kw.pop("sample_rate", SAMPLE_RATE))
        if transfer_kw:
            raise TypeError(f"transfer_and_score: unexpected arguments {sorted(transfer_kw)}")
        B, n_stats = waves.shape[0], len(inputs) - 3
        if reference is None:
            if n_reference is not None:
                raise ValueError("transfer_and_score: n_reference without reference")
            if mfcc:
                raise ValueError("transfer_and_score: mfcc=True scores against a reference, and none was given")
            if self_similarity:
                raise ValueError("transfer_and_score: self_similarity=True scores against a reference, and none was given")
            extra = []
        else:
            if not torch.is_tensor(reference) or reference.dim() != 2 or reference.dtype != torch.float32 or reference.shape[0] != B or \
                    not reference.is_cuda:
                raise ValueError(f"transfer_and_score: reference must be ({B}, m) float32 cuda rows")
            if n_reference is None:
                n_reference = torch.full((B,), reference.shape[1], dtype=torch.int32, device=reference.device)
            extra = [reference, len_tensor(n_reference, B, "n_reference", device=True)]

        def run(wav, cls, n, *rest):
            st, ref = rest[:n_stats], rest[n_stats:]
            if native is not None:                                   # score against what the models see: the clip at 22 050 Hz
                wav, n = U.resample_batch(wav, n, native, SAMPLE_RATE)
            out_wave, sections, lengths = self._run_wave(wav, cls, n, frames, st[:k] or None, st[k:] or None)
            scores = (M.mse_spectrogram(wav, out_wave, n, lengths),)
            if ref:
                scores += (M.instrumentation_similarity(out_wave, ref[0], lengths, ref[1]),)
                if mfcc:
                    scores += (M.mfcc_distance(out_wave, ref[0], lengths, ref[1]),)
            if chroma:
                scores += (M.chroma_similarity(out_wave, wav, lengths, n),)
            if onsets:
                scores += (M.onset_accuracy(wav, out_wave, n, lengths),)
            if self_similarity:
                scores += (M.self_similarity_distance(out_wave, ref[0], lengths, ref[1]),)
            return (out_wave, sections, lengths) + scores

        key += ("score", None if reference is None else tuple(reference.shape))
        if mfcc:
            key += ("mfcc",)
        if chroma:
            key += ("chroma",)
        if onsets:
            key += ("onsets",)
        if self_similarity:
            key += ("self_similarity",)
        res = self._replay(key, run, inputs + extra)
        names = ["mse_spectrogram"]                                  # in the order `run` appends them
        if reference is not None:
            names += ["instrumentation_similarity"] + (["mfcc_distance"] if mfcc else [])
        names += [name for flag, name in ((chroma, "chroma_similarity"), (onsets, "onset_accuracy"),
                                          (self_similarity, "self_similarity_distance")) if flag]
        return res[0], res[1], res[2], dict(zip(names, res[3:]))
