"""Drop-in for the reference's losses.py on libast_hip (single-workgroup
wavefront-reduction kernels; value and gradient from one launch each)."""
from __future__ import annotations

import torch

from . import ops
from ._lib import check, len_tensor, lib, ptr, stream


def _labels32(labels, device):
    if labels.is_cuda:
        return labels.to(torch.int32)
    return ops.const_tensor(tuple(int(v) for v in labels.tolist()), torch.int32, device)


def infoNCE_loss(style_emb: torch.Tensor, labels: torch.Tensor, temperature: float = 0.1) -> torch.Tensor:
    """losses.py:9-36."""
    return ops.InfoNCEFn.apply(style_emb, _labels32(labels, style_emb.device), float(temperature))


def margin_loss(class_emb: torch.Tensor, margin: float = 2.0, weight: float = 1.0) -> torch.Tensor:
    """losses.py:45-57 (`weight` is unused there too)."""
    return ops.MarginFn.apply(class_emb, float(margin))


def adversarial_loss(style_emb, class_emb, content_emb, discriminator, labels, compute_for_discriminator: bool,
                     lambda_content: float = 1.0, lambda_class: float = 0.5, lambda_style: float = 1.0):
    """losses.py:69-123."""
    dev = style_emb.device
    if content_emb.dim() == 3:
        content_emb = ops.mean_over_sections(content_emb)
    lab = _labels32(labels, dev)
    style_pred = discriminator(style_emb)
    content_pred = discriminator(content_emb)
    def wt(w, t):                         # a weight of exactly 1.0 needs no multiply launch
        return t if w == 1.0 else w * t
    d_loss = wt(lambda_style, ops.CrossEntropyFn.apply(style_pred, lab)) + wt(lambda_content, ops.CrossEntropyFn.apply(content_pred, lab))
    if class_emb is not None:
        class_pred = discriminator(class_emb)
        d_loss = d_loss + lambda_class * ops.CrossEntropyFn.apply(class_pred, ops.const_tensor((0, 1), torch.int32, dev))
    if compute_for_discriminator:
        return d_loss, None
    return d_loss, -wt(lambda_content, ops.SoftmaxEntropyFn.apply(content_pred))


def disentanglement_loss(style_emb: torch.Tensor, content_emb: torch.Tensor, use_hsic: bool = True, weight=20.0) -> torch.Tensor:
    """losses.py:138-191 (HSIC with the median heuristic, or the cross-covariance penalty; `weight` is unused there too)."""
    if not use_hsic:
        return ops.CrossCovFn.apply(style_emb, content_emb)
    return ops.HSICFn.apply(style_emb, content_emb)


# ---- validation: values only, for padded batches ---------------------------------------------------------------------------
RECON_KEYS = ("mse_loss", "mag_loss", "phase_loss", "temporal_loss", "spectral_loss")


def _spectrogram_arg(t, what, shape=None, who="reconstruction_losses"):
    """output / target of reconstruction_losses: (B, S, 2, T, F) float32 -> its shape"""
    if not torch.is_tensor(t) or t.dim() != 5 or t.dtype != torch.float32 or t.shape[2] != 2 or t.numel() == 0:
        got = f"{t.dtype} {tuple(t.shape)}" if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"{who}: {what} must be a non-empty (B, S, 2, T, F) float32 tensor, got {got}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{who}: {what} has shape {tuple(t.shape)}, output has {tuple(shape)}")
    return tuple(t.shape)


def _recon_len_args(who, ws_query, output, target, n_sections, lambda_temporal, lambda_phase, lambda_spectral, mse_weight):
    """The one argument check of the per-clip reconstruction losses -> (n_sections, target as a [..., :F] slice, its row stride,
    workspace floats, the five weights).  Every refusal is a ValueError that names `who` and the argument."""
    B, S, _, T, Fq = _spectrogram_arg(output, "output", who=who)
    _spectrogram_arg(target, "target", output.shape, who=who)
    n = len_tensor(n_sections, B, "n_sections", device=True, contiguous=True)
    for what, t in (("output", output), ("target", target)):
        if not t.is_cuda:
            raise ValueError(f"{who}: {what} must be on the GPU, got a tensor on {t.device} (there is no CPU path)")
    for name, v in (("lambda_temporal", lambda_temporal), ("lambda_phase", lambda_phase), ("lambda_spectral", lambda_spectral),
                    ("mse_weight", mse_weight)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v:
            raise ValueError(f"{who}: {name} must be a number, got {v!r}")
    need = int(ws_query(B, S, T, Fq))
    if need < 0:
        raise ValueError(f"{who}: output of shape {tuple(output.shape)} is out of range: {lib().ast_last_error().decode()}")
    tgt = target.detach()
    ld = tgt.stride(3)
    if tgt.stride(4) != 1 or ld < Fq or tuple(tgt.stride()[:3]) != (S * 2 * T * ld, 2 * T * ld, T * ld):
        tgt, ld = tgt.contiguous(), Fq               # anything but a [..., :F] slice of a contiguous tensor
    return n, tgt, ld, need, (float(mse_weight), 0.5, float(lambda_phase), float(lambda_temporal), float(lambda_spectral))


def _parts(res):
    parts = {"total_loss": res[:, 5]}
    parts.update({k: res[:, 6 + i] for i, k in enumerate(RECON_KEYS)})
    return parts


def reconstruction_losses(output, target, n_sections=None, lambda_temporal=0.3, lambda_phase=0.2, lambda_spectral=0.1, mse_weight=2.0):
    """compute_comprehensive_loss (new_decoder.py:348-420; mse_weight=1.0: SimpleDecoder_TransformerOnly.py:136-204) for every clip
    of a zero-padded batch by itself: entry b of each result is the reference's value for (output[b:b+1, :n_b], target[b:b+1, :n_b]),
    n_b = n_sections[b] clamped to [1, S] on the device (None: every clip holds S sections).  Sections s >= n_b of either tensor
    are not read, so they may hold anything.  Returns a dict of (B,) float32 device tensors under the reference's keys.  Values
    only: nothing here carries a gradient (training: ragged_reconstruction_loss).  No host read and no atomics
    (ast_recon_loss_len): the call can be captured, one graph serves every mix of lengths, and the values are bit-identical from
    run to run."""
    import ctypes as C
    n, tgt, ld, need, w5 = _recon_len_args("reconstruction_losses", lib().ast_recon_loss_len_ws_floats, output, target, n_sections,
                                           lambda_temporal, lambda_phase, lambda_spectral, mse_weight)
    B, S, _, T, Fq = output.shape
    out = output.detach().contiguous()
    ws = torch.empty(need, dtype=torch.float32, device=out.device)
    res = torch.empty((B, 11), dtype=torch.float32, device=out.device)
    check(lib().ast_recon_loss_len(ptr(out), ptr(tgt), ld, B, S, T, Fq, ptr(n), (C.c_float * 5)(*w5), ptr(ws), need, ptr(res), stream()),
          "ast_recon_loss_len")
    return _parts(res)


def ragged_reconstruction_loss(output, target, n_sections=None, clip_weights=None, lambda_temporal=0.3, lambda_phase=0.2,
                               lambda_spectral=0.1, mse_weight=2.0):
    """The training loss of a zero-padded batch of clips of different lengths: -> (loss, parts).
    loss = sum_b w_b * total_b, a 0-d tensor differentiable with respect to `output`; total_b is compute_comprehensive_loss of
    clip b alone, (output[b:b+1, :n_b], target[b:b+1, :n_b]) with n_b = n_sections[b] clamped to [1, S] on the device (None:
    every clip holds S sections), and w_b = clip_weights[b] (float32 (B,) device tensor; None: 1/B, the batch mean -- at equal
    lengths loss is then compute_comprehensive_loss(output, target)["total_loss"] and has its gradient).  parts is the dict of
    (B,) tensors of reconstruction_losses and carries no gradient.  The gradient rows of sections s >= n_b are exactly 0 and those
    sections of either tensor are never read.  One streaming pass computes values and gradient (ast_recon_loss_len_grad); no host
    read, no atomics: capturable, one graph for every mix of lengths, bit-identical from run to run.  As with the reference, the
    phase term's gradient is undefined where an output bin is exactly 0."""
    who = "ragged_reconstruction_loss"
    n, tgt, ld, _, w5 = _recon_len_args(who, lib().ast_recon_loss_len_grad_ws_floats, output, target, n_sections, lambda_temporal,
                                        lambda_phase, lambda_spectral, mse_weight)
    B = output.shape[0]
    cw = clip_weights
    if cw is not None:
        if not (torch.is_tensor(cw) and cw.dtype == torch.float32 and tuple(cw.shape) == (B,) and cw.is_cuda):
            got = f"{cw.dtype} {tuple(cw.shape)} on {cw.device}" if torch.is_tensor(cw) else type(cw).__name__
            raise ValueError(f"{who}: clip_weights must be a float32 device tensor of shape ({B},), got {got}")
        cw = cw.detach().contiguous()
    loss, res = ops.ReconLenGradFn.apply(output.contiguous(), tgt, ld, n, cw, w5)
    return loss, _parts(res)


def _value(dev, call, what):
    """call(loss) launches one loss kernel with null gradient pointers -> the scalar it wrote"""
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    check(call(loss), what)
    return loss[0]


def embedding_loss_values(style_emb, class_emb, content_mean, discriminator, labels, temperature=0.1, margin=2.0,
                          lambda_content=1.0, lambda_class=0.5, lambda_style=1.0):
    """The embedding losses of this file forward only (the same kernels with null gradient pointers), for a validation pass:
    -> dict of scalar device tensors nce, margin, hsic (HSIC with the median heuristic, the term the train step uses), adv_d, adv_g.
    content_mean: (B, d), the content embedding already averaged over each clip's own sections."""
    dev = style_emb.device
    s, c, k = style_emb.detach().contiguous(), content_mean.detach().contiguous(), class_emb.detach().contiguous()
    B, D = s.shape
    lab = _labels32(labels, dev)
    L = lib()
    ws = torch.empty(max(2 * B * B + B, 6 * B * B + 2 * B + 8), dtype=torch.float32, device=dev)      # InfoNCE's and HSIC's scratch
    out = {"nce": _value(dev, lambda o: L.ast_infonce(ptr(s), ptr(lab), B, D, float(temperature), ptr(o), None, ptr(ws), stream()), "ast_infonce"),
           "margin": _value(dev, lambda o: L.ast_margin(ptr(k), k.shape[0], k.shape[1], float(margin), ptr(o), None, stream()), "ast_margin")}
    out["hsic"] = _value(dev, lambda o: L.ast_hsic(ptr(s), ptr(c), B, D, ptr(o), None, None, ptr(ws), stream()), "ast_hsic")

    def ce(logits, target32):
        z = logits.contiguous()
        return _value(dev, lambda o: L.ast_cross_entropy(ptr(z), ptr(target32), z.shape[0], z.shape[1], ptr(o), None, stream()), "ast_cross_entropy")

    # losses.py:69-123 with the discriminator as it stands: its loss and the generator's entropy term from the same predictions
    content_pred = discriminator(c).contiguous()
    terms = [(lambda_style, ce(discriminator(s), lab)), (lambda_content, ce(content_pred, lab)),
             (lambda_class, ce(discriminator(k), ops.const_tensor((0, 1), torch.int32, dev)))]
    d_loss = None
    for w, t in terms:
        t = t if w == 1.0 else w * t
        d_loss = t if d_loss is None else d_loss + t
    ent = _value(dev, lambda o: L.ast_softmax_entropy(ptr(content_pred), content_pred.shape[0], content_pred.shape[1], ptr(o), None, stream()),
                 "ast_softmax_entropy")
    out["adv_d"], out["adv_g"] = d_loss, -(ent if lambda_content == 1.0 else lambda_content * ent)
    return out
