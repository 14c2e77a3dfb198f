"""Drop-in for the reference's SimpleDecoder_TransformerOnly.py (the decoder the shipped checkpoints / evaluation
scripts use): the CNN halves of new_decoder.Decoder replaced by two 2*287*513 x 256 linears around the
same pre-norm transformer decoder.  The two big linears stream their 301 MB f32 weights once per use through
ast_bigk_gemm / ast_skinny_gemm / ast_bign_dgrad / ast_linear_wgrad (no packed copies)."""
from __future__ import annotations

import torch
import torch.nn as nn

from . import layers as L
from . import ops
from .new_decoder import _comprehensive_loss
from .style_encoder import SinusoidalPositionalEncoding, _module_bank


class Decoder(nn.Module):
    """SimpleDecoder_TransformerOnly.py:9-133; identical attribute names and state_dict keys."""

    def __init__(self, d_model=256, nhead=4, num_layers=4, dim_feedforward=1024, dropout=0.1):
        super().__init__()
        self.d_model = d_model
        self.stft_dim = 2 * 287 * 513
        self.stft_to_embedding = nn.Linear(self.stft_dim, d_model)
        self.embedding_to_stft = nn.Linear(d_model, self.stft_dim)
        self.content_proj = nn.Linear(d_model, d_model)
        self.class_proj = nn.Linear(d_model, d_model)
        self.pos_encoding = SinusoidalPositionalEncoding(d_model)
        layer = nn.TransformerDecoderLayer(d_model=d_model, nhead=nhead, dim_feedforward=dim_feedforward, dropout=dropout,
                                           batch_first=True, norm_first=True)
        self.transformer_decoder = nn.TransformerDecoder(layer, num_layers=num_layers)
        self.start_token = nn.Parameter(torch.randn(1, 1, d_model))
        self.input_norm = nn.LayerNorm(d_model)
        self.output_norm = nn.LayerNorm(d_model)
        self.dropout = nn.Dropout(dropout)
        self._init_weights()

    def _init_weights(self):
        """SimpleDecoder_TransformerOnly.py:46-54 (same rule as new_decoder.py:134-143)."""
        for name, p in self.named_parameters():
            if "weight" in name:
                nn.init.xavier_uniform_(p, gain=0.2) if p.dim() > 1 else nn.init.zeros_(p)
            elif "bias" in name:
                nn.init.zeros_(p)

    def register(self, bank):
        lin = lambda l: bank.add(l.weight, "linear", L.tok_dtype, bias=l.bias)  # noqa: E731
        self._cp, self._kp = lin(self.content_proj), lin(self.class_proj)
        self._layers = [L.DecoderLayer(bank, l) for l in self.transformer_decoder.layers]

    def _prepare(self):
        _module_bank(self).prepare(self.training)

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

    def generate_output(self, decoder_outputs):
        """SimpleDecoder_TransformerOnly.py:62-66."""
        return self._generate(decoder_outputs)

    def create_causal_mask(self, seq_len, device=None):
        return torch.triu(torch.ones(seq_len, seq_len, device=device), diagonal=1).bool()

    def _memory(self, content_emb, class_emb):
        B, Sc, D = content_emb.shape
        if 2 * Sc > ops.ATTN_MAX_L:
            raise ValueError(f"{Sc} content sections make {2 * Sc} memory tokens; the attention core takes {ops.ATTN_MAX_L} "
                             f"(at most {ops.ATTN_MAX_L // 2} sections per clip)")
        cm = L.linear(content_emb.reshape(B * Sc, D), self._cp).view(B, Sc, D)
        km = L.linear(class_emb, self._kp).unsqueeze(1).expand(-1, Sc, -1)
        return ops.dropout(torch.cat([cm, km], dim=1), self.dropout.p, self.training)

    def _check_lengths(self, lengths, B):
        if lengths is None:
            return
        if self.training:
            raise ValueError("per-clip lengths are an inference feature: call .eval() first (training takes equal-length batches)")
        if lengths.dtype != torch.int32 or tuple(lengths.shape) != (B,):
            raise ValueError(f"lengths must be an int32 tensor of shape ({B},), got {lengths.dtype} {tuple(lengths.shape)}")

    def prepare_memory(self, content_emb, class_emb, lengths=None):
        """SimpleDecoder_TransformerOnly.py:72-78.  With per-clip lengths (int32 (B,), inference) the memory keeps its padded
        shape (B, 2 Sc, d): pass the same lengths to forward_inference, whose cross-attention skips the padded tokens of
        both halves."""
        self._check_lengths(lengths, content_emb.shape[0])
        self._prepare()
        return self._memory(content_emb, class_emb)

    def _stack(self, tgt, memory, lengths=None):
        if lengths is not None:
            for lyr in self._layers:
                tgt = lyr(tgt, memory, self.training, lengths)
            return tgt
        for lyr in self._layers:
            tgt = lyr(tgt, memory, self.training)
        return tgt

    def _training_pass(self, y, memory):
        B = y.shape[0]
        emb = self._encode(y)
        tgt = torch.cat([self.start_token.expand(B, 1, -1), emb[:, :-1, :]], dim=1)
        tgt = L.layer_norm(self.pos_encoding(tgt), self.input_norm)
        return self._generate(self._stack(tgt, memory))

    def forward_training(self, y, memory):
        """SimpleDecoder_TransformerOnly.py:80-102."""
        self._prepare()
        return self._training_pass(y, memory)

    # How forward_inference walks the sequence, as in new_decoder.Decoder: "recompute" = the reference's loop
    # (SimpleDecoder_TransformerOnly.py:104-125: the whole stack over all tokens generated so far, every step); "kv_cache" = one
    # new token per step against cached per-layer K/V (the layers are causal), taken only when grad is disabled.
    decode_mode = "recompute"

    def _inference_pass_cached(self, memory, target_length, lengths=None):
        B = memory.size(0)
        mem_kv = [lyr.memory_kv(memory) for lyr in self._layers]
        caches = [None] * len(self._layers)
        tok = self.start_token.expand(B, -1, -1)
        pe = self.pos_encoding.pe
        outs = []
        for t in range(target_length):
            x = tok + pe[:, t:t + 1]
            for i, lyr in enumerate(self._layers):
                x, caches[i] = lyr.step(x, caches[i], mem_kv[i]) if lengths is None else lyr.step(x, caches[i], mem_kv[i], lengths)
            outs.append(x)
            tok = x
        return self._generate(torch.cat(outs, dim=1), lengths)

    def _inference_pass(self, memory, target_length=None, lengths=None):
        """lengths were checked by the caller (forward / forward_inference, before the weights are prepared)."""
        B = memory.size(0)
        if target_length is None:
            target_length = memory.size(1) // 2
        if target_length > self.pos_encoding.pe.size(1):
            raise ValueError(f"target_length {target_length}, but the positional table holds "
                             f"{self.pos_encoding.pe.size(1)} positions")
        if self.decode_mode == "kv_cache" and not torch.is_grad_enabled():
            return self._inference_pass_cached(memory, target_length, lengths)
        seq = self.start_token.expand(B, -1, -1)
        outs = []
        for _ in range(target_length):
            nxt = self._stack(self.pos_encoding(seq), memory, lengths)[:, -1:, :]
            outs.append(nxt)
            seq = torch.cat([seq, nxt], dim=1)
        return self._generate(torch.cat(outs, dim=1), lengths)

    def forward_inference(self, memory, target_length=None, lengths=None):
        """SimpleDecoder_TransformerOnly.py:104-125.  lengths: see forward."""
        self._check_lengths(lengths, memory.size(0))
        self._prepare()
        return self._inference_pass(memory, target_length, lengths)

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
