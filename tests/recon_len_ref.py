"""Float64 numpy reference of the per-clip reconstruction loss of a padded batch (ast_recon_loss_len, include/ast_hip.h;
ast_amd.reconstruction_losses): this file defines the expected values.  Row b is compute_comprehensive_loss
(new_decoder.py:348-420; mse_weight 1.0: SimpleDecoder_TransformerOnly.py:136-204) of (out[b:b+1, :n_b], tgt[b:b+1, :n_b]) with
n_b = clamp(n_sections[b], 1, S).  tests/test_validation_cpu.py holds it to oracle.ast_oracle.comprehensive_loss, which
tests/golden/ pins to the real reference; the GPU tests then measure the kernel against it.  Also here: the case table and the
seeded inputs both test files share."""
import numpy as np

KEYS = ("mse_loss", "mag_loss", "phase_loss", "temporal_loss", "spectral_loss")
WEIGHTS = {"new": 2.0, "simple": 1.0}            # new_decoder.py:406, SimpleDecoder_TransformerOnly.py:194


def clamp_sections(n_sections, B, S):
    if n_sections is None:
        return np.full(B, S, dtype=np.int64)
    return np.clip(np.asarray(n_sections, dtype=np.int64), 1, S)


def recon_len_ref(out, tgt, n_sections=None, lambda_temporal=0.3, lambda_phase=0.2, lambda_spectral=0.1, mse_weight=2.0):
    """out, tgt (B, S, 2, T, F) -> (B, 11) float64: [5 raw sums][total][5 means], the layout of the kernel's result.  Sections
    s >= n_b are sliced away before anything is computed, so whatever they hold (NaN included) cannot reach a result; a term
    without elements (temporal at n_b == 1, axis-3 difference at T == 1) is exactly 0."""
    out, tgt = np.asarray(out, dtype=np.float64), np.asarray(tgt, dtype=np.float64)
    B, S, C, T, F = out.shape
    assert C == 2 and tgt.shape == out.shape
    res = np.zeros((B, 11))
    w = (mse_weight, 0.5, lambda_phase, lambda_temporal, lambda_spectral)
    for b, n in enumerate(clamp_sections(n_sections, B, S)):
        o, g = out[b, :n], tgt[b, :n]
        e = o - g
        mo = np.sqrt(o[:, 0] ** 2 + o[:, 1] ** 2 + 1e-8)
        mt = np.sqrt(g[:, 0] ** 2 + g[:, 1] ** 2 + 1e-8)
        dphi = np.arctan2(o[:, 1], o[:, 0]) - np.arctan2(g[:, 1], g[:, 0])
        dphi = np.mod(dphi + np.pi, 2 * np.pi) - np.pi                       # torch.remainder: the sign of the divisor
        sums = [np.sum(e ** 2), np.sum((mo - mt) ** 2), np.sum(dphi ** 2),
                np.sum((e[1:] - e[:-1]) ** 2) if n > 1 else 0.0,
                np.sum((e[:, :, 1:] - e[:, :, :-1]) ** 2) if T > 1 else 0.0]
        counts = [2 * n * T * F, n * T * F, n * T * F, 2 * (n - 1) * T * F, 2 * n * (T - 1) * F]
        means = [s / c if c > 0 else 0.0 for s, c in zip(sums, counts)]
        res[b, :5], res[b, 6:] = sums, means
        res[b, 5] = sum(wk * m for wk, m in zip(w, means))
    return res


def recon_batch_ref(out, tgt, coef5, dtype=None):
    """The batch form with its gradient (ast_recon_loss, ast_recon_loss_total): out, tgt (B, S, 2, T, F) torch tensors ->
    (the five raw sums over the WHOLE batch, total = sum_k coef5[k] * sums[k], d total / d out), evaluated in `dtype`
    (default float64; float32 gives the plain single-precision evaluation the GPU tests measure their tolerance with).  The
    sums are those of recon_len_ref with every clip full, added over the clips; a term without elements is an empty sum, 0,
    and sends no gradient.  The gradient is autograd's, so where a bin of `out` is exactly 0 it is whatever atan2's is."""
    import math
    import torch
    dt = dtype or torch.float64
    o = out.detach().to(dt).clone().requires_grad_(True)
    g = tgt.detach().to(dt)
    e = o - g
    mo = torch.sqrt(o[:, :, 0] ** 2 + o[:, :, 1] ** 2 + 1e-8)
    mt = torch.sqrt(g[:, :, 0] ** 2 + g[:, :, 1] ** 2 + 1e-8)
    dphi = torch.atan2(o[:, :, 1], o[:, :, 0]) - torch.atan2(g[:, :, 1], g[:, :, 0])
    dphi = torch.remainder(dphi + math.pi, 2 * math.pi) - math.pi
    sums = [(e ** 2).sum(), ((mo - mt) ** 2).sum(), (dphi ** 2).sum(),
            ((e[:, 1:] - e[:, :-1]) ** 2).sum(), ((e[:, :, :, 1:] - e[:, :, :, :-1]) ** 2).sum()]
    total = sum(float(c) * s for c, s in zip(coef5, sums))
    (grad,) = torch.autograd.grad(total, o)
    return torch.stack([s.detach() for s in sums]), total.detach(), grad


# ---- the cases of tests/test_gpu_validation.py: (name, B, S, T, F, row stride of the target, n_sections or None) ----------------
CASES = (
    ("small-ragged", 3, 3, 5, 7, 9, (3, 1, 2)),       # an unpadded clip, a one-section clip, a clip whose last real section is followed by padding
    ("small-full", 3, 3, 5, 7, 9, None),
    ("real-size", 2, 2, 287, 513, 597, (2, 1)),        # 576 workgroups per clip: the finishing launch's lanes wrap over the slots
    ("strided-bins", 1, 2, 3, 400000, 400000, (2,)),   # 1.2 M bins per clip > 4096 workgroups x 256: threads stride over several bins
)


def make_case(B, S, T, F, ld, seed=0):
    """Seeded (out, x) float32 with x (B, S, 2, T, ld) and the target its [..., :F] view.  Magnitudes ~ N(0, 1); phases drawn so
    that the wrapped difference takes both signs of torch.remainder's branch (out near +pi against tgt near -pi and the other way
    round, in a tenth of the bins each); |out| = 0 exactly in about 1 % of the bins, where the 1e-8 under the root decides."""
    g = np.random.default_rng(1000 + seed)
    shape = (B, S, T, F)
    mag_o, mag_t = np.abs(g.standard_normal(shape)) + 0.05, np.abs(g.standard_normal(shape)) + 0.05
    ph_o, ph_t = g.uniform(-np.pi, np.pi, shape), g.uniform(-np.pi, np.pi, shape)
    u = g.random(shape)
    edge = g.uniform(0.02, 0.3, shape)
    ph_o = np.where(u < 0.1, np.pi - edge, np.where(u < 0.2, -np.pi + edge, ph_o))
    ph_t = np.where(u < 0.1, -np.pi + edge[..., ::-1], np.where(u < 0.2, np.pi - edge[..., ::-1], ph_t))
    mag_o = np.where(g.random(shape) < 0.01, 0.0, mag_o)
    out = np.stack([mag_o * np.cos(ph_o), mag_o * np.sin(ph_o)], axis=2).astype(np.float32)
    out[out == 0] = 0.0                               # +0 in both parts: atan2(+-0, -0) is +-pi, atan2(+0, +0) is 0 everywhere
    x = (0.5 * g.standard_normal((B, S, 2, T, ld))).astype(np.float32)
    x[..., :F] = np.stack([mag_t * np.cos(ph_t), mag_t * np.sin(ph_t)], axis=2).astype(np.float32)
    return out, x
