"""Float64 numpy references of ragged training of the simple decoder: this file defines the expected values.

ragged_loss_ref: loss = sum_b w_b total_b and d loss / d out for a zero-padded batch (ast_recon_loss_len_grad, include/ast_hip.h;
ast_amd.ragged_reconstruction_loss), written as formulas.  total_b is compute_comprehensive_loss (new_decoder.py:348-420; mse_weight
1.0: SimpleDecoder_TransformerOnly.py:136-204) of (out[b:b+1, :n_b], tgt[b:b+1, :n_b]), n_b = clamp(n_sections[b], 1, S);
tests/test_ragged_train_cpu.py holds value and gradient to torch.autograd on oracle.ast_oracle.comprehensive_loss clip by clip.
masked_dgrad_ref / masked_wgrad_ref: the backward of the length-masked output linear (ast_bign_dgrad_len, ast_linear_wgrad_len)
as plain matrix products over the rows that count.  Also here: the case tables and seeded inputs both test files share."""
import numpy as np

from recon_len_ref import clamp_sections, recon_len_ref

WEIGHT_DEFAULTS = dict(lambda_temporal=0.3, lambda_phase=0.2, lambda_spectral=0.1, mse_weight=2.0)
MIN_MAG = 0.05              # |out| and |tgt| of every bin of make_grad_case: the reference's phase gradient is NaN at 0
WRAP_MARGIN = 0.01          # rad: the wrapped phase difference stays this far from +-pi, so f32 and f64 take the same branch


def ragged_loss_ref(out, tgt, n_sections=None, clip_weights=None, lambda_temporal=0.3, lambda_phase=0.2, lambda_spectral=0.1, mse_weight=2.0):
    """out, tgt (B, S, 2, T, F) -> (loss, grad (B, S, 2, T, F) float64 = d loss / d out, res (B, 11) of recon_len_ref).
    Rows s >= n_b of grad are exactly 0 and those sections of out / tgt are sliced away before anything is computed.  A term without
    elements (temporal at n_b == 1, axis-3 difference at T == 1) has coefficient 0."""
    out, tgt = np.asarray(out, dtype=np.float64), np.asarray(tgt, dtype=np.float64)
    B, S, C, T, F = out.shape
    res = recon_len_ref(out, tgt, n_sections, lambda_temporal, lambda_phase, lambda_spectral, mse_weight)
    w = np.full(B, 1.0 / B) if clip_weights is None else np.asarray(clip_weights, dtype=np.float64)
    weights = (mse_weight, 0.5, lambda_phase, lambda_temporal, lambda_spectral)
    grad = np.zeros_like(out)
    for b, n in enumerate(clamp_sections(n_sections, B, S)):
        o, g = out[b, :n], tgt[b, :n]
        counts = (2 * n * T * F, n * T * F, n * T * F, 2 * (n - 1) * T * F, 2 * n * (T - 1) * F)
        c = [w[b] * wk / ck if ck > 0 else 0.0 for wk, ck in zip(weights, counts)]
        e = o - g
        mo2 = o[:, 0] ** 2 + o[:, 1] ** 2
        mo, mt = np.sqrt(mo2 + 1e-8), np.sqrt(g[:, 0] ** 2 + g[:, 1] ** 2 + 1e-8)
        dphi = np.arctan2(o[:, 1], o[:, 0]) - np.arctan2(g[:, 1], g[:, 0])
        dphi = np.mod(dphi + np.pi, 2 * np.pi) - np.pi
        gph = np.stack([-o[:, 1] / mo2, o[:, 0] / mo2], axis=1)            # d atan2(im, re) / d (re, im)
        gt, gs = np.zeros_like(e), np.zeros_like(e)                         # d/de of sum (e[s+1] - e[s])^2 / 2, along sections and along axis 3
        if n > 1:
            d = e[1:] - e[:-1]
            gt[1:] += d
            gt[:-1] -= d
        if T > 1:
            d = e[:, :, 1:] - e[:, :, :-1]
            gs[:, :, 1:] += d
            gs[:, :, :-1] -= d
        grad[b, :n] = 2.0 * (c[0] * e + c[1] * ((mo - mt) / mo)[:, None] * o + c[2] * dphi[:, None] * gph + c[3] * gt + c[4] * gs)
    return float(np.sum(w * res[:, 5])), grad, res


def make_grad_case(B, S, T, F, ld, seed=0):
    """Seeded (out, x) float32 like recon_len_ref.make_case, but fit for gradients: every |out|, |tgt| >= MIN_MAG, and the wrapped
    phase difference is drawn from [-pi + 2 WRAP_MARGIN, pi - 2 WRAP_MARGIN] with the target's phase uniform, so the raw difference
    leaves (-pi, pi] on either side in about a quarter of the bins each (both signs of torch.remainder's branch)."""
    g = np.random.default_rng(2000 + seed)
    shape = (B, S, T, F)
    mag_o, mag_t = np.abs(g.standard_normal(shape)) + 2 * MIN_MAG, np.abs(g.standard_normal(shape)) + 2 * MIN_MAG
    ph_t = g.uniform(-np.pi, np.pi, shape)
    delta = g.uniform(-np.pi + 2 * WRAP_MARGIN, np.pi - 2 * WRAP_MARGIN, shape)
    ph_o = np.mod(ph_t + delta + np.pi, 2 * np.pi) - np.pi
    out = np.stack([mag_o * np.cos(ph_o), mag_o * np.sin(ph_o)], axis=2).astype(np.float32)
    x = (0.5 * g.standard_normal((B, S, 2, T, ld))).astype(np.float32)
    x[..., :F] = np.stack([mag_t * np.cos(ph_t), mag_t * np.sin(ph_t)], axis=2).astype(np.float32)
    return out, x


def case_properties(out, tgt):
    """(smallest |out|, smallest distance of the wrapped phase difference from +-pi, raw difference above pi somewhere, below -pi
    somewhere) in float64 on the float32 inputs: what make_grad_case promises."""
    o, t = np.asarray(out, dtype=np.float64), np.asarray(tgt, dtype=np.float64)
    raw = np.arctan2(o[:, :, 1], o[:, :, 0]) - np.arctan2(t[:, :, 1], t[:, :, 0])
    wrapped = np.mod(raw + np.pi, 2 * np.pi) - np.pi
    return (float(np.sqrt(o[:, :, 0] ** 2 + o[:, :, 1] ** 2).min()), float((np.pi - np.abs(wrapped)).min()),
            bool((raw > np.pi).any()), bool((raw < -np.pi).any()))


def seeded_clip_weights(B, seed=0):
    return np.random.default_rng(3000 + seed).uniform(0.2, 1.5, B).astype(np.float32)


# ---- the loss cases of tests/test_gpu_ragged_train.py: (name, B, S, T, F, row stride of the target, n_sections or None) ---------
LOSS_CASES = (
    ("small-ragged", 3, 3, 5, 7, 9, (3, 1, 2)),
    ("small-full", 3, 3, 5, 7, 9, None),
    ("one-frame", 2, 2, 1, 7, 7, (2, 1)),              # T == 1: the axis-3 term has no elements
    ("strided-bins", 1, 2, 3, 400000, 400000, (2,)),   # 1.2 M bins per clip > 4096 workgroups x 256: threads stride
    ("real-size", 2, 2, 287, 513, 597, (2, 1)),
)


def loss_case(name):
    _, B, S, T, F, ld, n = next(c for c in LOSS_CASES if c[0] == name)
    out, x = make_grad_case(B, S, T, F, ld, seed=len(name))
    return out, x, F, ld, n


# ---- the masked output linear's backward ------------------------------------------------------------------------------------
def row_mask(M, S, n_valid):
    """(M,) bool: row m = b S + s counts iff s < clamp(n_valid[b], 1, S)"""
    n = clamp_sections(n_valid, M // S, S)
    return (np.arange(M) % S) < np.repeat(n, S)


def masked_dgrad_ref(dy, w, S, n_valid):
    """dx[m] = dy[m] @ w for the rows that count, exactly 0 elsewhere (those rows of dy are never looked at)"""
    dy, w = np.asarray(dy, dtype=np.float64), np.asarray(w, dtype=np.float64)
    keep = row_mask(dy.shape[0], S, n_valid)
    dx = np.zeros((dy.shape[0], w.shape[1]))
    dx[keep] = dy[keep] @ w
    return dx


def masked_wgrad_ref(dy, x, S, n_valid):
    """(dW, db) = (dy^T x, column sums of dy) over the rows that count"""
    dy, x = np.asarray(dy, dtype=np.float64), np.asarray(x, dtype=np.float64)
    keep = row_mask(dy.shape[0], S, n_valid)
    return dy[keep].T @ x[keep], dy[keep].sum(axis=0)


# (M, S, n_valid): one tile; across the 64-row workgroup boundary into a workgroup without a counting row; whole 16-row tiles and a
# whole workgroup dead; no mask
LINEAR_ROWS = ((9, 3, (3, 1, 2)), (68, 17, (17, 1, 16, 5)), (130, 65, (65, 1)), (130, 65, None))
LINEAR_N, LINEAR_KS = 2050, (256, 100)              # four 512-chunks of n with a tail of 2


def linear_case(M, N, K, seed=0):
    """seeded float32 (dy (M, N), w (N, K), x (M, K), dW0 (N, K), db0 (N,))"""
    g = np.random.default_rng(4000 + seed)
    f = lambda *s: g.standard_normal(s).astype(np.float32)      # noqa: E731
    return f(M, N), (f(N, K) / np.sqrt(K)).astype(np.float32), f(M, K), f(N, K), f(N)
