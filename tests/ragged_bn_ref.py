"""Float64 references for BatchNorm over the live images of a padded batch and for new_decoder.Decoder.forward_training_ragged_bn.

Images are the N = B * S sections of B clips, image n = b * S + s; n_b = clamp(n_sections[b], 1, S); image n is live iff s < n_b.
The masked BatchNorm+ReLU is written out as formulas over the live images (tests/test_ragged_bn_cpu.py holds them to
torch.nn.BatchNorm2d under autograd on the index-selected live images); the decoder reference runs oracle.ast_oracle's two CNN
halves on the CONCATENATION of the live sections of all clips and its transformer clip by clip (the "compaction" reference)."""
import numpy as np
import torch

from oracle import ast_oracle as O

EPS = 1e-5
MOMENTUM = 0.1

# (B, S, H, W, C, Creal, n_sections): the smallest shapes at which each path of the kernels can go wrong
BN_CASES = (
    ("one-unit", 3, 3, 5, 7, 8, 8, (3, 1, 2)),              # one 8-channel unit; 35 pixels: not a multiple of a workgroup's share
    ("eight-units", 2, 2, 9, 4, 64, 64, (2, 1)),            # the widest decoder layer
    ("padded-channels", 1, 2, 4, 4, 8, 1, (1,)),            # Creal < C: padded channels must come out with scale 0
    ("130-images", 2, 65, 3, 3, 16, 16, (65, 1)),           # the finalize's lanes stride past 64 rows; 64 dead rows in a stretch
    ("clamped", 2, 3, 4, 4, 8, 8, (0, 9)),                  # lengths outside [1, S]: clamped on the device
    ("full", 2, 3, 4, 4, 8, 8, (3, 3)),                     # every image live: ops.BatchNormActFn on the same input
)
BN_NAMES = [c[0] for c in BN_CASES]


def bn_case(name):
    return next(c[1:] for c in BN_CASES if c[0] == name)


def clamp_sections(n_sections, B, S):
    n = np.full(B, S, dtype=np.int64) if n_sections is None else np.asarray(n_sections, dtype=np.int64)
    return np.clip(n, 1, S)


def live_mask(B, S, n_sections):
    """bool (B * S,): image b * S + s is live iff s < n_b"""
    return (np.arange(S)[None, :] < clamp_sections(n_sections, B, S)[:, None]).reshape(-1)


def bn_inputs(name, seed=0):
    """x, dy (N, Creal, H, W) float32 NCHW; gamma, beta, running_mean, running_var (Creal,) float32: seeded, with a mean and a spread
    that differ between live and dead images, so statistics over all images miss the reference by far"""
    B, S, H, W, C, Creal, n = bn_case(name)
    g = torch.Generator().manual_seed(1000 + 17 * seed + len(name))
    N = B * S
    x = torch.randn(N, Creal, H, W, generator=g) * 2.0 + 0.5
    dead = torch.from_numpy(~live_mask(B, S, n))
    x[dead] = x[dead] * 3.0 - 4.0
    dy = torch.randn(N, Creal, H, W, generator=g)
    gamma = torch.empty(Creal).uniform_(0.5, 1.5, generator=g)
    beta = torch.randn(Creal, generator=g) * 0.2
    rm = torch.randn(Creal, generator=g) * 0.1
    rv = torch.empty(Creal).uniform_(0.5, 1.5, generator=g)
    return x, dy, gamma, beta, rm, rv


def masked_bn_relu_fwd(x, gamma, beta, rm, rv, live, relu=True):
    """x (N, C, H, W); live bool (N,).  -> y (dead images 0), mean, biased variance, new running_mean, new running_var; float64."""
    x, gamma, beta, rm, rv = (np.asarray(a, dtype=np.float64) for a in (x, gamma, beta, rm, rv))
    xl = x[live]
    cnt = xl.shape[0] * xl.shape[2] * xl.shape[3]
    mean = xl.sum(axis=(0, 2, 3)) / cnt
    var = (xl * xl).sum(axis=(0, 2, 3)) / cnt - mean * mean
    rstd = 1.0 / np.sqrt(var + EPS)
    y = (x - mean[None, :, None, None]) * (gamma * rstd)[None, :, None, None] + beta[None, :, None, None]
    if relu:
        y = np.maximum(y, 0.0)
    y[~live] = 0.0
    new_rm = (1.0 - MOMENTUM) * rm + MOMENTUM * mean
    new_rv = (1.0 - MOMENTUM) * rv + MOMENTUM * var * cnt / max(cnt - 1, 1)
    return y, mean, var, new_rm, new_rv


def masked_bn_relu_bwd(x, dy, gamma, beta, live, relu=True):
    """-> dx (dead images 0), dgamma, dbeta; float64.  dz = dy under the ReLU mask of the live images;
    dx = gamma rstd (dz - mean(dz) - xhat mean(dz xhat)) with the means over the live pixels."""
    x, dy, gamma, beta = (np.asarray(a, dtype=np.float64) for a in (x, dy, gamma, beta))
    xl = x[live]
    cnt = xl.shape[0] * xl.shape[2] * xl.shape[3]
    mean = xl.sum(axis=(0, 2, 3)) / cnt
    var = (xl * xl).sum(axis=(0, 2, 3)) / cnt - mean * mean
    rstd = 1.0 / np.sqrt(var + EPS)
    b = lambda v: v[None, :, None, None]                                   # noqa: E731
    xhat = (x - b(mean)) * b(rstd)
    dz = np.where(live[:, None, None, None], dy, 0.0)
    if relu:
        dz = np.where(xhat * b(gamma) + b(beta) > 0.0, dz, 0.0)
    dbeta = dz.sum(axis=(0, 2, 3))
    dgamma = (dz * xhat).sum(axis=(0, 2, 3))
    dx = b(gamma * rstd) * (dz - b(dbeta) / cnt - xhat * b(dgamma) / cnt)
    dx[~live] = 0.0
    return dx, dgamma, dbeta


# ---- the decoder ---------------------------------------------------------------------------------------------------------------------
def double_state(sd):
    """an oracle state dict in float64 (parameters keep requires_grad)"""
    return {k: (v.detach().double().requires_grad_(v.requires_grad) if v.is_floating_point() else v.clone()) for k, v in sd.items()}


def compaction_decoder(sd, content, class_emb, y, n_sections, nhead=4, nlayers=4):
    """What forward_training_ragged_bn computes: oracle.ast_oracle's decoder with both CNN halves on the concatenated live sections
    of all clips (one image batch of sum_b n_b sections) and the transformer on each clip alone.  content (B, S, d), class_emb
    (B, d), y (B, S, 2, 287, 513); sd as oracle.layout.seeded_model_state("decoder") (any float dtype; mutated like one training
    forward: spectral-norm vectors and BatchNorm running statistics).  -> (B, S, 2, 287, 513), sections s >= n_b zero."""
    cfg = O.Cfg(training=True, p_drop=0.0)
    B, S = y.shape[:2]
    nb = clamp_sections(n_sections, B, S)
    emb = O.decoder_encode_input(sd, torch.cat([y[b, :nb[b]] for b in range(B)], dim=0), cfg)
    d = emb.shape[-1]
    toks, off = [], 0
    for b in range(B):
        k = int(nb[b])
        memory = O.decoder_prepare_memory(sd, content[b:b + 1, :k], class_emb[b:b + 1], cfg)
        tgt = torch.cat([sd["start_token"], emb[off:off + k - 1][None]], dim=1)
        tgt = O.layernorm(sd, "input_norm.", tgt + O.positional_encoding(k, d))
        toks.append(O._decoder_stack(sd, tgt, memory, nhead, nlayers, cfg)[0])
        off += k
    live = O.decoder_generate_output(sd, torch.cat(toks, dim=0)[None], cfg)[0]
    rows, off = [], 0
    for b in range(B):
        k = int(nb[b])
        rows.append(torch.cat([live[off:off + k], live.new_zeros(S - k, *live.shape[1:])], dim=0))
        off += k
    return torch.stack(rows, dim=0)


def ragged_loss(out, y, n_sections, mse_weight=2.0):
    """mean over the clips of oracle.comprehensive_loss of clip b alone on its n_b sections (ast_amd.ragged_reconstruction_loss with
    clip_weights None), differentiable"""
    B, S = out.shape[:2]
    nb = clamp_sections(n_sections, B, S)
    return sum(O.comprehensive_loss(out[b:b + 1, :nb[b]], y[b:b + 1, :nb[b]], mse_weight=mse_weight)["total_loss"] for b in range(B)) / B


def decoder_inputs(B, S, seed=0):
    """content (B, S, 256), class_emb (B, 256), y (B, S, 2, 287, 513): seeded float32"""
    g = torch.Generator().manual_seed(4200 + 31 * seed + 7 * B + S)
    return torch.randn(B, S, 256, generator=g), torch.randn(B, 256, generator=g), 0.5 * torch.randn(B, S, 2, 287, 513, generator=g)
