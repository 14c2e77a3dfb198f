"""Drop-in for the reference's new_decoder.py (Decoder, compute_comprehensive_loss) on libast_hip."""
from __future__ import annotations

import torch
import torch.nn as nn
from torch.nn.utils import spectral_norm

from . import layers as L
from . import ops
from .decoder_trunk import DecoderTrunk, bank_linear

ENC_CH = ((2, 16, 1), (16, 32, 2), (32, 64, 2), (64, 64, 2))        # (cin, cout, stride)  new_decoder.py:29-48
DEC_CH = ((1, 64), (64, 32), (32, 16), (16, 8))                      # stride-2 transposed convs  new_decoder.py:72-93


def _conv_bn_relu_slots(conv, ch):
    return [conv, nn.BatchNorm2d(ch), nn.Identity()]      # slot 3 is the (parameter-free) ReLU


class Decoder(DecoderTrunk):
    """new_decoder.py:9-345: a CNN pair around the shared transformer decoder (decoder_trunk.DecoderTrunk).  Sequential slot
    numbering is kept so state_dict keys match (conv_encoder.0/1/3/4/..., spatial_projection.0/1/3, conv_decoder.0/1/.../12)."""

    token_programs = True             # _stack may take tokprog.decoder_stack; the simple decoder never does

    def __init__(self, d_model=256, nhead=4, num_layers=4, dim_feedforward=1024, dropout=0.1, max_seq_len=1000):
        super().__init__()
        self.max_seq_len = max_seq_len
        self.F_compressed, self.T_compressed, self.feature_dim = 32, 16, 64
        enc = []
        for cin, cout, s in ENC_CH:
            enc += _conv_bn_relu_slots(spectral_norm(nn.Conv2d(cin, cout, kernel_size=3, stride=s, padding=1)), cout)
        enc.append(nn.AdaptiveAvgPool2d((self.F_compressed, self.T_compressed)))
        self.conv_encoder = nn.Sequential(*enc)
        fd = self.feature_dim
        self.spatial_projection = nn.Sequential(
            *_conv_bn_relu_slots(spectral_norm(nn.Conv2d(fd, fd, kernel_size=3, padding=1)), fd),
            spectral_norm(nn.Conv2d(fd, 1, kernel_size=1)))
        self.feature_to_sequence = nn.Linear(self.F_compressed * self.T_compressed, d_model)
        self.sequence_to_feature = nn.Linear(d_model, self.F_compressed * self.T_compressed)
        dec = []
        for cin, cout in DEC_CH:
            dec += _conv_bn_relu_slots(
                spectral_norm(nn.ConvTranspose2d(cin, cout, kernel_size=3, stride=2, padding=1, output_padding=1)), cout)
        dec.append(spectral_norm(nn.ConvTranspose2d(8, 2, kernel_size=3, padding=1)))
        dec.append(nn.Upsample(size=(287, 513), mode="bilinear", align_corners=False))
        self.conv_decoder = nn.Sequential(*dec)
        self._build_trunk(d_model, nhead, num_layers, dim_feedforward, dropout)
        self._init_weights()

    # ---- weight registration ------------------------------------------------------
    def register(self, bank):
        conv = lambda c: bank.add(c.weight_orig, "conv", L.img_dtype, u=c.weight_u, v=c.weight_v, bias=c.bias)  # noqa: E731
        convt = lambda c: bank.add(c.weight_orig, "convT", L.img_dtype, u=c.weight_u, v=c.weight_v, bias=c.bias)  # noqa: E731
        self._enc = [conv(self.conv_encoder[i]) for i in (0, 3, 6, 9)]
        self._sp = [conv(self.spatial_projection[0]), conv(self.spatial_projection[3])]
        self._dec = [convt(self.conv_decoder[i]) for i in (0, 3, 6, 9, 12)]
        self._f2s, self._s2f = bank_linear(bank, self.feature_to_sequence), bank_linear(bank, self.sequence_to_feature)
        super().register(bank)

    # ---- CNN halves -----------------------------------------------------------------
    # One body per half for the plain pass and for the padded-batch training pass (forward_training_ragged_bn).  live = None: the
    # plain layers.  live = (n_sections, S): every BatchNorm over the live images only (layers.conv_bn_act_len /
    # convT_bn_act_len, training mode) and the masked bilinear.  What keeps dead images out of every result then:
    # - every BatchNorm and the bilinear store exact zeros for dead images, forward (y) and backward (dx), without loading them;
    # - so a dead image contributes 0 x (finite) to every weight and bias gradient, PROVIDED what it holds is finite.  It is not
    #   always zero: a bias-carrying convolution turns a dead image of zeros into its bias before the next BatchNorm zeroes it
    #   again, and conv_decoder[0] reads sequence_to_feature of the stack's dead token rows, which are finite but not zero.
    #   Finite they are: the masked layout conversion feeds zeros, not the caller's padding, into conv_encoder[0].
    def _bn_layers(self, live):
        """(conv+BN+ReLU, convT+BN+ReLU) as callables (h, pw, stride, bn) for this pass"""
        tr = self.training
        if live is None:
            return (lambda h, pw, s, bn: L.conv_bn_act(h, pw, 3, s, 1, bn, tr, relu=True),
                    lambda h, pw, s, bn: L.convT_bn_act(h, pw, 3, s, 1, 1, bn, tr, relu=True))
        return (lambda h, pw, s, bn: L.conv_bn_act_len(h, pw, 3, s, 1, bn, live),
                lambda h, pw, s, bn: L.convT_bn_act_len(h, pw, 3, s, 1, 1, bn, live))

    def _encode_nhwc(self, h, live=None):
        conv_bn, _ = self._bn_layers(live)
        for pw, i, (_, _, s) in zip(self._enc, (0, 3, 6, 9), ENC_CH):
            h = conv_bn(h, pw, s, self.conv_encoder[i + 1])
        h = ops.AdaptivePoolFn.apply(h, self.F_compressed, self.T_compressed)
        h = conv_bn(h, self._sp[0], 1, self.spatial_projection[1])
        h = L.conv(h, self._sp[1], 1, 1, 0, True)                          # (N,32,16,8): channel 0 is the real one
        flat = ops.CastFn.apply(h[..., 0].reshape(h.shape[0], -1), torch.float32)
        return L.linear(flat, self._f2s)

    def encode_input(self, x):
        """new_decoder.py:145-168: (N,2,287,513) f32 -> (N,d_model)."""
        self._prepare()
        return self._encode_nhwc(ops.nchw_to_nhwc(x, L.img_dtype()))

    def _generate(self, tok, lengths=None, live=None):
        """lengths (inference) is accepted and ignored: without `live` the CNN takes every section, so output sections
        s >= lengths[b] are finite and unspecified.  live = (n_sections, S), training: see the note above _bn_layers; output
        sections of dead images are exact 0."""
        B, S, D = tok.shape
        _, convT_bn = self._bn_layers(live)
        h = L.linear(L.layer_norm(tok, self.output_norm).reshape(B * S, D), self._s2f)       # (N,512) f32
        h = ops.CastFn.apply(h, L.img_dtype()).view(B * S, self.F_compressed, self.T_compressed, 1)
        h = torch.cat([h, h.new_zeros(B * S, self.F_compressed, self.T_compressed, 7)], dim=3)   # pad C 1 -> 8
        for pw, i in zip(self._dec[:4], (0, 3, 6, 9)):
            h = convT_bn(h, pw, 2, self.conv_decoder[i + 1])
        h = L.convT(h, self._dec[4], 3, 1, 1, 0, True)                                      # (N,512,256,8)
        out = ops.BilinearToNCHWFn.apply(h, 2, 287, 513) if live is None else ops.BilinearToNCHWLenFn.apply(h, 2, 287, 513, *live)
        return out.view(B, S, 2, 287, 513)

    def _check_ragged(self):
        raise NotImplementedError("new_decoder.Decoder.forward_training_ragged does not exist: the BatchNorm layers of its CNNs couple "
                                  "the clips of a batch, so 'what the clips give one by one' cannot hold.  forward_training_ragged_bn "
                                  "trains on a padded batch with BatchNorm statistics over the real sections "
                                  "(SimpleDecoder_TransformerOnly.Decoder has forward_training_ragged)")

    # ---- training on a padded batch: BatchNorm statistics over the real sections ---------------------------------------------------
    def forward_training_ragged_bn(self, content_emb, class_emb, y, n_sections):
        """The teacher-forced training pass on a zero-padded batch of clips of different lengths, with the BatchNorm statistics of
        both CNN halves taken over the real sections only.  Arguments and contract as DecoderTrunk.forward_training_ragged:
        content_emb (B, S, d), class_emb (B, d), y (B, S, 2, 287, 513), n_sections an int32 (B,) device tensor, clip b holding
        n_b = clamp(n_sections[b], 1, S) real sections (clamped and counted on the device: one captured graph serves every mix of
        lengths); training mode only; at most WIDE_MAX_ROWS token rows; output sections s >= n_b exactly 0; padded sections of y
        may hold anything (NaN included); padded rows of content_emb must be finite; the loss must give rows s >= n_b no gradient
        (ast_amd.ragged_reconstruction_loss).

        The semantics DIFFER from the simple decoder's forward_training_ragged.  BatchNorm couples the clips of a batch, so the
        result is NOT what the clips give one by one.  It is what the reference decoder gives when its two CNN halves see the
        concatenation of the real sections of all clips as their image batch (sum_b n_b images: batch statistics, running
        statistics and gradients over exactly those) and the transformer sees each clip alone.  For B = 1, and for a batch at full
        lengths, that is the reference's forward_training.

        Dead images are not zero everywhere inside the pass (see the note above _bn_layers): correctness rests on every BatchNorm
        and the bilinear storing exact 0 for them in both directions, and on what they hold staying finite.

        Every BatchNorm runs ops.BatchNormActLenFn, which takes the separate per-image statistics passes whatever config says and
        raises ValueError under sync-BN and in deterministic mode."""
        n = self._ragged_args("forward_training_ragged_bn", content_emb, y, n_sections,
                              lambda: ops.check_bn_len_supported("forward_training_ragged_bn"))
        self._prepare()
        B, S = y.shape[:2]
        live = (n, S)
        memory = self._memory(content_emb, class_emb)
        emb = self._encode_nhwc(ops.nchw_to_nhwc_len(y.view(B * S, *y.shape[2:]), L.img_dtype(), n, S), live)
        return self._generate(self._shifted_stack(emb.view(B, S, self.d_model), memory, n), live=live)

    def generate_output(self, decoder_outputs):
        """new_decoder.py:170-193."""
        self._prepare()
        return self._generate(decoder_outputs)

    def create_causal_mask(self, seq_len):
        return torch.triu(torch.ones(seq_len, seq_len), diagonal=1).bool()

    def _embed_target(self, y):
        B, S = y.shape[:2]
        return self._encode_nhwc(ops.nchw_to_nhwc(y.view(B * S, *y.shape[2:]), L.img_dtype())).view(B, S, self.d_model)

    def encode_target(self, y):
        """Teacher-forcing embeddings of the target sections (new_decoder.py:246-248).  Independent of the
        encoders, so the trainer runs it on its own stream; pass the result to forward(y_embeddings=...)."""
        self._prepare()
        return self._embed_target(y)

    def _training_pass(self, y, memory, y_embeddings=None, lengths=None):
        return self._teacher_forced(self._embed_target(y) if y_embeddings is None else y_embeddings, memory, lengths)

    def forward(self, content_emb, class_emb, y=None, target_length=None, y_embeddings=None, lengths=None):
        """new_decoder.py:321-345 (+ optional precomputed encode_target(y)).
        lengths: None, or an int32 (B,) device tensor for a padded batch at inference (eval mode, torch.no_grad()): clip b
        holds lengths[b] real sections, and its cross-attention sees content and class tokens s < lengths[b] only.  Output
        sections s >= lengths[b] are finite and unspecified."""
        self._check_lengths(lengths, content_emb.shape[0])
        if y_embeddings is None or not (self.training and y is not None):
            self._prepare()
        memory = self._memory(content_emb, class_emb)
        if self.training and y is not None:
            if len(y.shape) != 5:
                raise ValueError(f"Expected y to have shape [B, S, 2, 287, 513], got {y.shape}")
            return self._training_pass(y, memory, y_embeddings)
        return self._inference_pass(memory, target_length, lengths)


def compute_comprehensive_loss(output, target, lambda_temporal=0.3, lambda_phase=0.2, lambda_spectral=0.1):
    """new_decoder.py:348-420 as ONE streaming kernel pass (value + gradient).  Only `total_loss`
    carries gradient; the component entries are detached values."""
    return _comprehensive_loss(output, target, lambda_temporal, lambda_phase, lambda_spectral, 2.0)


def _comprehensive_loss(output, target, lambda_temporal, lambda_phase, lambda_spectral, mse_weight):
    B, S, _, Freq, T = output.shape
    n = B * S * Freq * T
    c = (mse_weight / (2 * n), 0.5 / n, lambda_phase / n,
         (lambda_temporal / (2 * B * (S - 1) * Freq * T)) if S > 1 else 0.0,
         (lambda_spectral / (2 * B * S * (Freq - 1) * T)) if Freq > 1 else 0.0)
    # the five reported components are sums * 1/count, formed by the same finishing launch as the total (they carry no gradient)
    inv = (1.0 / (2 * n), 1.0 / n, 1.0 / n,
           1.0 / (2 * B * (S - 1) * Freq * T) if S > 1 else 0.0,
           1.0 / (2 * B * S * (Freq - 1) * T) if Freq > 1 else 0.0)
    total, _, parts = ops.ReconTotalFn.apply(output.contiguous(), target, c, inv)
    return {"total_loss": total, "mse_loss": parts[0], "mag_loss": parts[1], "phase_loss": parts[2],
            "temporal_loss": parts[3], "spectral_loss": parts[4]}
