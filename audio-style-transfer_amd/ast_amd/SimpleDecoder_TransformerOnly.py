"""Drop-in for the reference's SimpleDecoder_TransformerOnly.py (the decoder the shipped checkpoints / evaluation
scripts use): the CNN halves of new_decoder.Decoder replaced by two 2*287*513 x 256 linears around the
same pre-norm transformer decoder.  The two big linears stream their 301 MB f32 weights once per use through
ast_bigk_gemm / ast_skinny_gemm / ast_bign_dgrad / ast_linear_wgrad (no packed copies)."""
from __future__ import annotations

import torch
import torch.nn as nn

from . import layers as L
from . import ops
from .decoder_trunk import DecoderTrunk
from .new_decoder import _comprehensive_loss


class Decoder(DecoderTrunk):
    """SimpleDecoder_TransformerOnly.py:9-133; identical attribute names and state_dict keys.  The transformer between the two big
    linears is decoder_trunk.DecoderTrunk, whose bank entries are the only packed weights (register is the trunk's)."""

    def __init__(self, d_model=256, nhead=4, num_layers=4, dim_feedforward=1024, dropout=0.1):
        super().__init__()
        self.stft_dim = 2 * 287 * 513
        self.stft_to_embedding = nn.Linear(self.stft_dim, d_model)
        self.embedding_to_stft = nn.Linear(d_model, self.stft_dim)
        self._build_trunk(d_model, nhead, num_layers, dim_feedforward, dropout)
        self._init_weights()

    # ---- the two big linears ---------------------------------------------------------
    def _encode(self, x):
        B, S = x.shape[:2]
        flat = x.contiguous().reshape(B * S, -1)
        return ops.BigLinearFn.apply(flat, self.stft_to_embedding.weight, self.stft_to_embedding.bias).view(B, S, self.d_model)

    def encode_input(self, x):
        """SimpleDecoder_TransformerOnly.py:56-60: (B,S,2,287,513) -> (B,S,d_model)."""
        return self._encode(x)

    def _generate(self, tok, lengths=None):
        """Training, and inference up to WIDE_MAX_ROWS rows without lengths: BigLinearFn.  With per-clip lengths, or past that row
        count under no_grad: ops.big_out_linear (up to BIGN_MAX_ROWS rows; sections s >= lengths[b] come back as exactly 0)."""
        B, S, D = tok.shape
        h = L.layer_norm(tok, self.output_norm).reshape(B * S, D)
        lin = self.embedding_to_stft
        if lengths is not None or (B * S > ops.WIDE_MAX_ROWS and not torch.is_grad_enabled()):
            return ops.big_out_linear(h, lin.weight, lin.bias, S, lengths).view(B, S, 2, 287, 513)
        return ops.BigLinearFn.apply(h, lin.weight, lin.bias).view(B, S, 2, 287, 513)

    # ---- the same two for DecoderTrunk.forward_training_ragged: no BatchNorm here, only the two linears need the lengths ----------
    def _check_ragged(self):
        pass

    def _encode_ragged(self, y, n_sections):
        """_encode whose weight gradient skips the rows of padded sections (ast_linear_wgrad_len): they are user data."""
        B, S = y.shape[:2]
        lin = self.stft_to_embedding
        return ops.BigLinearFn.apply(y.contiguous().reshape(B * S, -1), lin.weight, lin.bias, S, n_sections).view(B, S, self.d_model)

    def _generate_ragged(self, tok, n_sections):
        B, S, D = tok.shape
        lin = self.embedding_to_stft
        h = L.layer_norm(tok, self.output_norm).reshape(B * S, D)
        return ops.BigOutLinearLenFn.apply(h, lin.weight, lin.bias, S, n_sections).view(B, S, 2, 287, 513)

    def generate_output(self, decoder_outputs):
        """SimpleDecoder_TransformerOnly.py:62-66."""
        return self._generate(decoder_outputs)

    def create_causal_mask(self, seq_len, device=None):
        return torch.triu(torch.ones(seq_len, seq_len, device=device), diagonal=1).bool()

    def _training_pass(self, y, memory, lengths=None):
        return self._teacher_forced(self._encode(y), memory, lengths)

    def forward(self, content_emb, class_emb, y=None, target_length=None, lengths=None):
        """SimpleDecoder_TransformerOnly.py:127-133.
        lengths: None, or an int32 (B,) device tensor for a padded batch at inference (eval mode, torch.no_grad()): clip b holds
        lengths[b] real sections (clamped to [1, S] on the device), and its cross-attention sees content and class tokens
        s < lengths[b] only.  Output sections s >= lengths[b] are exactly 0."""
        self._check_lengths(lengths, content_emb.shape[0])
        self._prepare()
        memory = self._memory(content_emb, class_emb)
        if self.training and y is not None:
            return self._training_pass(y, memory)
        return self._inference_pass(memory, target_length, lengths)


def compute_comprehensive_loss(output, target, lambda_temporal=0.3, lambda_phase=0.2, lambda_spectral=0.1):
    """SimpleDecoder_TransformerOnly.py:136-204: new_decoder's loss with the MSE term weighted 1.0 (:194) instead of
    2.0 (new_decoder.py:406); same single-pass kernel."""
    return _comprehensive_loss(output, target, lambda_temporal, lambda_phase, lambda_spectral, 1.0)
