"""The transformer decoder that new_decoder.Decoder and SimpleDecoder_TransformerOnly.Decoder share (the reference writes it out in
both files: new_decoder.py:104-143,208-319 and SimpleDecoder_TransformerOnly.py:20-54,72-125).  The two differ only in how STFT
sections become tokens and how tokens become sections; a subclass builds those modules around one call of `_build_trunk` and
supplies `_generate(tok, lengths)`.  Everything between is here once: memory, the layer stack, teacher forcing, both ways of walking
the sequence at inference, and the per-clip `lengths` of a padded batch."""
from __future__ import annotations

import torch
import torch.nn as nn

from . import layers as L
from . import config, ops, tokprog
from ._lib import len_tensor
from .style_encoder import SinusoidalPositionalEncoding, _module_bank


def bank_linear(bank, lin: nn.Linear):
    return bank.add(lin.weight, "linear", L.tok_dtype, bias=lin.bias)


class DecoderTrunk(nn.Module):
    # Whether _stack may run as one token program (tokprog.decoder_stack) when config.tok_programs enables them.
    token_programs = False

    # How forward_inference walks the sequence: "recompute" = the reference's loop (new_decoder.py:294-314,
    # SimpleDecoder_TransformerOnly.py:104-125: the whole stack over all tokens generated so far, every step); "kv_cache" = one new
    # token per step against cached per-layer K/V (identical results: the layers are causal), taken only when grad is disabled.
    # Class attribute so callers and tests can switch it.
    decode_mode = "recompute"

    def _build_trunk(self, d_model, nhead, num_layers, dim_feedforward, dropout):
        """The trunk's modules, in the reference's order: construction draws from the global generator, and _init_weights and the
        state_dict follow registration order.  A subclass builds its own modules first, then calls this, then _init_weights()."""
        self.d_model = d_model
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

    def _init_weights(self):
        """new_decoder.py:134-143, SimpleDecoder_TransformerOnly.py:46-54: Xavier-uniform(gain 0.2) for >=2-D `*weight*`, zeros for
        1-D weights and biases (so a fresh decoder outputs exactly 0 -- SURVEY F7)."""
        for name, p in self.named_parameters():
            if "weight" in name:
                nn.init.xavier_uniform_(p, gain=0.2) if p.dim() > 1 else nn.init.zeros_(p)
            elif "bias" in name:
                nn.init.zeros_(p)

    def register(self, bank):
        """The trunk's bank entries; a subclass with packed weights of its own adds them first and then calls this."""
        self._cp, self._kp = bank_linear(bank, self.content_proj), bank_linear(bank, self.class_proj)
        self._layers = [L.DecoderLayer(bank, l) for l in self.transformer_decoder.layers]

    def _prepare(self):
        _module_bank(self).prepare(self.training)

    def _check_lengths(self, lengths, B):
        """Every public entry point calls this before it prepares the weight bank."""
        len_tensor(lengths, B, "lengths", training=self.training)

    def _memory(self, content_emb, class_emb):
        B, Sc, D = content_emb.shape
        if 2 * Sc > ops.ATTN_MAX_L:
            raise ValueError(f"{Sc} content sections make {2 * Sc} memory tokens; the attention core takes {ops.ATTN_MAX_L} "
                             f"(at most {ops.ATTN_MAX_L // 2} sections per clip)")
        cm = L.linear(content_emb.reshape(B * Sc, D), self._cp).view(B, Sc, D)
        km = L.linear(class_emb, self._kp).unsqueeze(1).expand(-1, Sc, -1)
        return ops.dropout(torch.cat([cm, km], dim=1), self.dropout.p, self.training)

    def prepare_memory(self, content_emb, class_emb, lengths=None):
        """new_decoder.py:208-229, SimpleDecoder_TransformerOnly.py:72-78.  With per-clip lengths (int32 (B,), inference) the memory
        keeps its padded shape (B, 2 Sc, d): pass the same lengths to forward_inference, whose cross-attention skips the padded
        tokens of both halves."""
        self._check_lengths(lengths, content_emb.shape[0])
        self._prepare()
        return self._memory(content_emb, class_emb)

    def _stack(self, tgt, memory, lengths=None):
        """The decoder layers over tgt, as tokprog.run_encoder_stack does it for the encoders: one token program where the class
        allows them, they are enabled and take this shape, else layer by layer.  lengths always goes layer by layer: the token
        programs have no key mask."""
        if (self.token_programs and lengths is None and config.tok_programs > 0
                and tokprog.decoder_stack_ok(tgt, memory, self._layers)):
            return tokprog.decoder_stack(tgt, memory, self._layers, self.training)
        for lyr in self._layers:
            tgt = lyr(tgt, memory, self.training, lengths)
        return tgt

    def _teacher_forced(self, emb, memory, lengths=None):
        """emb (B, S, d), the embedded target sections: shifted right behind the start token, through the stack, to sections
        (the second half of forward_training: new_decoder.py:231-269, SimpleDecoder_TransformerOnly.py:80-102).  lengths (a padded
        batch, eval mode): clip b's target tokens s >= lengths[b] are replaced by zeros first -- the causal self-attention gives
        them weight 0 in every real row, and 0 times whatever a padded target section embeds to must stay 0 -- and the
        cross-attention sees the clip's own memory tokens only."""
        return self._generate(self._shifted_stack(emb, memory, lengths), lengths)

    def _shifted_stack(self, emb, memory, lengths=None):
        """_teacher_forced up to the stack's output tokens (B, S, d)."""
        if lengths is not None:
            S = emb.shape[1]
            keep = torch.arange(S, device=emb.device)[None, :] < lengths.clamp(1, S)[:, None]
            emb = torch.where(keep[:, :, None], emb, torch.zeros_like(emb))
        tgt = torch.cat([self.start_token.expand(emb.shape[0], 1, -1), emb[:, :-1, :]], dim=1)
        tgt = L.layer_norm(self.pos_encoding(tgt), self.input_norm)
        return self._stack(tgt, memory, lengths)

    # ---- training on a padded batch of clips of different lengths ------------------------------------------------------------------
    def _check_ragged(self):
        """Subclass hook: return if this decoder has _encode_ragged and _generate_ragged, else raise NotImplementedError saying why.
        _encode_ragged(y, n_sections): target sections (B, S, 2, 287, 513) -> (B, S, d) with nothing of sections s >= n_sections[b]
        reaching a parameter gradient; _generate_ragged(tok, n_sections): stack output (B, S, d) -> sections, rows s >= n_sections[b]
        exactly 0."""
        raise NotImplementedError(f"{type(self).__module__}.{type(self).__name__} has no length-aware training pass")

    def forward_training_ragged(self, content_emb, class_emb, y, n_sections):
        """The teacher-forced training pass (forward_training) on a zero-padded batch of clips of different lengths.
        content_emb (B, S, d), class_emb (B, d), y (B, S, 2, 287, 513) the target sections, n_sections an int32 (B,) device tensor:
        clip b holds n_b = n_sections[b] real sections (clamped to [1, S] on the device, no host read: one captured graph serves
        every mix of lengths).  Training mode only (eval mode: forward_teacher_forced(..., lengths=)).  Output rows s < n_b, and
        with ast_amd.ragged_reconstruction_loss on top every gradient, are what the clips give one by one.
        - Output sections s >= n_b are exactly 0.
        - Padded sections of y may hold anything (NaN included): their embeddings are replaced by zeros and the weight gradient of
          the embedding never reads them.
        - Padded rows of content_emb must be finite: the cross-attention never sees them, but the weight gradient of their
          projection multiplies them by an exact 0.
        The loss must give rows s >= n_b no gradient, as ragged_reconstruction_loss does."""
        n = self._ragged_args("forward_training_ragged", content_emb, y, n_sections, self._check_ragged)
        self._prepare()
        memory = self._memory(content_emb, class_emb)
        return self._generate_ragged(self._shifted_stack(self._encode_ragged(y, n), memory, n), n)

    def _ragged_args(self, who, content_emb, y, n_sections, check_supported=None):
        """The argument checks every ragged training entry point makes, in this order and before the weight bank is prepared:
        training mode, the subclass's own refusal (check_supported), y's rank, the row cap, n_sections (len_tensor).  Returns
        n_sections, contiguous.  (forward_training_ragged used to look at n_sections before y's rank and the row cap; a call that
        is wrong in both now gets the shape error first -- the shape checks need no device tensor.)"""
        if not self.training:
            raise ValueError(f"{who} is the training pass: call .train() first "
                             "(in eval mode a padded batch goes through forward_teacher_forced(..., lengths=))")
        if check_supported is not None:
            check_supported()
        if y.dim() != 5:
            raise ValueError(f"Expected y to have shape [B, S, 2, 287, 513], got {tuple(y.shape)}")
        if y.shape[0] * y.shape[1] > ops.WIDE_MAX_ROWS:
            raise RuntimeError(f"{who}: {y.shape[0] * y.shape[1]} token rows > {ops.WIDE_MAX_ROWS} "
                               "(the cap of the wide token path, AST_WIDE_MAX_ROWS)")
        B = content_emb.shape[0]
        if n_sections is None:
            raise ValueError(f"n_sections must be an int32 device tensor of shape ({B},), got None")
        return len_tensor(n_sections, B, "n_sections", device=True, contiguous=True)

    def forward_training(self, y, memory):
        """new_decoder.py:231-269, SimpleDecoder_TransformerOnly.py:80-102."""
        self._prepare()
        return self._training_pass(y, memory)

    def forward_teacher_forced(self, content_emb, class_emb, y, lengths=None):
        """The teacher-forced pass of forward_training on (content_emb, class_emb) in whatever mode the module is in: in eval mode
        under torch.no_grad() it gives the validation output comparable to the training loss (forward() in eval mode decodes
        autoregressively, as the reference does: new_decoder.py:337-345).  y (B, S, 2, 287, 513): the target sections.
        lengths: None, or an int32 (B,) device tensor for a zero-padded batch (eval mode only): clip b holds lengths[b] real
        sections; its rows s < lengths[b] are what the clip gives alone, the rest is as forward() documents."""
        self._check_lengths(lengths, content_emb.shape[0])
        if y.dim() != 5:
            raise ValueError(f"Expected y to have shape [B, S, 2, 287, 513], got {tuple(y.shape)}")
        self._prepare()
        return self._training_pass(y, self._memory(content_emb, class_emb), lengths=lengths)

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
                x, caches[i] = lyr.step(x, caches[i], mem_kv[i], lengths)
            outs.append(x)
            tok = x
        return self._generate(torch.cat(outs, dim=1), lengths)

    def _inference_pass(self, memory, target_length=None, lengths=None):
        """lengths were checked by the caller (forward / forward_inference, before the weights are prepared)."""
        B = memory.size(0)
        if target_length is None:
            target_length = memory.size(1) // 2
        if target_length > self.pos_encoding.pe.size(1):
            raise ValueError(f"target_length {target_length}, but the positional table holds {self.pos_encoding.pe.size(1)} positions")
        if self.decode_mode == "kv_cache" and not torch.is_grad_enabled():
            return self._inference_pass_cached(memory, target_length, lengths)
        seq = self.start_token.expand(B, -1, -1)
        outs = []
        for _ in range(target_length):
            nxt = self._stack(self.pos_encoding(seq), memory, lengths)[:, -1:, :]      # no input_norm here (new_decoder.py:296)
            outs.append(nxt)
            seq = torch.cat([seq, nxt], dim=1)
        return self._generate(torch.cat(outs, dim=1), lengths)

    def forward_inference(self, memory, target_length=None, lengths=None):
        """new_decoder.py:272-319, SimpleDecoder_TransformerOnly.py:104-125.  lengths: see the subclass's forward."""
        self._check_lengths(lengths, memory.size(0))
        self._prepare()
        return self._inference_pass(memory, target_length, lengths)
