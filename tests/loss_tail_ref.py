"""Float64 references of the tail of a training step, written as formulas, plus the case tables and seeded inputs that
tests/test_loss_tail_cpu.py (no GPU) and tests/test_gpu_loss_tail.py share: the embedding losses and cross-entropy / softmax-entropy
of csrc/losses.hip, ast_scale, and the step scalars, sum of squares and Adam of csrc/optim.hip.

Where oracle/ast_oracle.py is dtype-generic the float64 reference IS the oracle on float64 tensors: infonce_loss, margin_loss,
disentanglement_loss(use_hsic=False) and comprehensive_loss stay in float64 end to end (test_loss_tail_cpu.py checks the result
dtype and that nothing was rounded through float32).  The oracle's HSIC branch does not: it builds the centring matrix with
torch.eye(B), which is float32, so `hsic64` writes the formula out here.  Gradients are float64 autograd.

The kernels take float32 hyper-parameters (lr, betas, eps, wd, temperature, margin ...), so every reference evaluates its formula at
the float32-rounded value of each: the function and its inputs are the kernel's, only the arithmetic is float64.

Tolerances are measured, never chosen (`bound`): e32 = max |plain float32 evaluation - float64| / max |float64| on the same inputs,
and the kernel must be within max(8 * e32, 64 * 2^-24) of the float64 result, relative to its max-abs.  8 covers the fast
__expf / __logf intrinsics and another summation order; the floor is the rounding of a 64-lane partial sum and applies where the
float32 evaluation happens to be exact."""
from __future__ import annotations

import math

import numpy as np
import torch

from oracle import ast_oracle as O

U24 = 2.0 ** -24
FLOOR = 64 * U24
FACTOR = 8.0
F64 = torch.float64


def f32(v):
    """the double that equals float32(v): what a `float` argument of the C ABI holds"""
    return float(np.float32(v))


def rel(a, ref):
    """max |a - ref| / max |ref| in float64 (rel_err of tests/test_gpu_ops.py)"""
    a, ref = torch.as_tensor(a).detach().double().cpu().reshape(-1), torch.as_tensor(ref).detach().double().cpu().reshape(-1)
    return float((a - ref).abs().max() / max(float(ref.abs().max()), 1e-300))


def bound(plain32, ref):
    """(e32, tolerance) for one compared quantity"""
    e32 = rel(plain32, ref)
    return e32, max(FACTOR * e32, FLOOR)


def is_zero(ref):
    return float(torch.as_tensor(ref).abs().max()) == 0.0


# ---- row losses ----------------------------------------------------------------------------------------------------------

def cross_entropy(logits, target):
    """mean over rows of logsumexp(z_r) - z_r[target_r]"""
    lse = torch.logsumexp(logits, dim=-1)
    return (lse - logits.gather(1, target.long()[:, None]).squeeze(1)).mean()


def softmax_entropy(logits):
    """mean over rows of -sum_k p_k log(p_k + 1e-8), p = softmax(z): the 1e-8 sits inside the log (losses.py:118-120)"""
    p = torch.softmax(logits, dim=-1)
    return -(p * torch.log(p + 1e-8)).sum(-1).mean()


def with_grad(fn, *xs, dtype=F64):
    """fn on detached copies of xs in `dtype` -> (value, gradients); a gradient nothing flows to is zeros"""
    xs = [x.detach().to(dtype).clone().requires_grad_(True) for x in xs]
    v = fn(*xs)
    if v.requires_grad:
        gs = torch.autograd.grad(v, xs, allow_unused=True)
    else:
        gs = [None] * len(xs)
    return v.detach(), [torch.zeros_like(x) if g is None else g for x, g in zip(xs, gs)]


# ---- embedding losses ----------------------------------------------------------------------------------------------------

def infonce(style, labels, temperature=0.1):
    return O.infonce_loss(style, labels, f32(temperature) if style.dtype == F64 else temperature)


def margin(cls, m=2.0):
    return O.margin_loss(cls, m)


def crosscov(style, content):
    return O.disentanglement_loss(style, content, use_hsic=False)


def hsic_rank(B):
    """0-based ascending rank of sigma in the flattened (2B)^2 distance matrix, diagonal included: the lower median"""
    return (2 * B) ** 2 // 2 - 1


def pair_distances(style, content):
    """(2B, 2B) float64 distances of the rows of [style; content], formed from differences (exact zeros on the diagonal)"""
    X = torch.cat([style, content], 0).double()
    return torch.cdist(X, X, compute_mode="donot_use_mm_for_euclid_dist")


def hsic64(style, content):
    """losses.py:138-191: sigma = the lower-median entry of the (2B)^2 distance matrix of [style; content] (gradient flows through
    it), K = exp(-|s_i - s_j|^2 / 2 sigma^2), L the same on content, HSIC = tr(K H L H) / (B - 1)^2 with H = I - 1/B."""
    B = style.shape[0]
    X = torch.cat([style, content], 0)
    dist = torch.cdist(X, X, compute_mode="donot_use_mm_for_euclid_dist")       # backward is 0 at zero distance
    flat = dist.flatten()
    order = torch.argsort(flat.detach(), stable=True)
    sigma = flat[order[hsic_rank(B)]]
    H = torch.eye(B, dtype=style.dtype) - 1.0 / B
    K = torch.exp(-dist[:B, :B] ** 2 / (2 * sigma ** 2))
    L = torch.exp(-dist[B:, B:] ** 2 / (2 * sigma ** 2))
    return torch.trace((K @ H) @ (L @ H)) / ((B - 1) ** 2)


def hsic_median_gap(style, content):
    """Relative distance from sigma to the nearest distance of a DIFFERENT pair (every off-diagonal distance occurs twice,
    as (i, j) and (j, i); the diagonal zeros count as one more value)."""
    d = pair_distances(style, content)
    M = d.shape[0]
    flat, _ = torch.sort(d.flatten())
    sigma = float(flat[hsic_rank(M // 2)])
    iu = torch.triu_indices(M, M, 1)
    pairs = torch.cat([d[iu[0], iu[1]], torch.zeros(1, dtype=F64)])
    gaps = (pairs - sigma).abs()
    same = int((gaps == 0).sum())
    assert same >= 1
    if same > 1:
        return 0.0
    return float(gaps[gaps > 0].min()) / sigma


# ---- step scalars, sum of squares, scale, Adam ---------------------------------------------------------------------------

def weighted_sum(terms, widx, weights):
    """sum_i w_i term_i, w_i = weights[widx_i], or 1 where widx_i < 0 -> (value, [w_i])"""
    w = [1.0 if i < 0 else float(weights[i]) for i in widx]
    return math.fsum(wi * float(t) for wi, t in zip(w, terms)), w


def sumsq(x):
    return float((x.double() ** 2).sum())


def scale(x, y, hscale, dscale, accumulate):
    """y (+)= hscale * dscale * x in float64 (dscale None: 1)"""
    sc = f32(hscale) * (1.0 if dscale is None else float(dscale))
    r = sc * x.double()
    return y.double() + r if accumulate else r


def clip_factor(gnorm_sq, max_norm):
    """min(1, max_norm / (sqrt(gnorm_sq) + 1e-6)); 1 without a norm or with max_norm <= 0"""
    if gnorm_sq is None or not max_norm > 0:
        return 1.0
    return min(1.0, max_norm / (math.sqrt(gnorm_sq) + f32(1e-6)))


def adam_step(p, g, m, v, step, lr, b1, b2, eps, wd, gnorm_sq=None, max_norm=0.0):
    """One step of adam_kernel in float64, as it writes it: the clipped gradient, wd * p added to it, m and v, the bias corrections
    1 - beta^step, eps outside the root.  -> (p, m, v)"""
    lr, b1, b2, eps, wd, max_norm = (f32(a) for a in (lr, b1, b2, eps, wd, max_norm))
    gi = g.double() * clip_factor(gnorm_sq, max_norm)
    if wd != 0:
        gi = gi + wd * p
    m = b1 * m + (1 - b1) * gi
    v = b2 * v + (1 - b2) * gi * gi
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    return p - lr * (m / bc1) / (torch.sqrt(v / bc2) + eps), m, v


# ---- the batch reconstruction loss -----------------------------------------------------------------------------------------

def recon_coefs(B, S, T, Fq, mse_weight=2.0, lambda_temporal=0.3, lambda_phase=0.2, lambda_spectral=0.1):
    """(coef5, inv5) of new_decoder.compute_comprehensive_loss: weight_k / count_k and 1 / count_k; a term without elements gets 0"""
    n = B * S * T * Fq
    nt, ns = 2 * B * (S - 1) * T * Fq, 2 * B * S * (T - 1) * Fq
    inv = (1.0 / (2 * n), 1.0 / n, 1.0 / n, 1.0 / nt if nt else 0.0, 1.0 / ns if ns else 0.0)
    w = (mse_weight, 0.5, lambda_phase, lambda_temporal, lambda_spectral)
    return tuple(a * b for a, b in zip(w, inv)), inv


# ---- cases and seeded inputs ---------------------------------------------------------------------------------------------

SUMSQ_N = (1, 3, 4, 1027, 786433 + 3, 900001, 1048576 + 7, 3000003)
SUMSQ_SLOTS = (1, 16, 256)


def sumsq_input(n):
    """randn times a slow ramp: the squares differ by position, so a dropped or doubled accumulator lane changes the sum"""
    g = torch.Generator().manual_seed(4000 + n % 9973)
    return torch.randn(n, generator=g) * torch.linspace(0.5, 2.0, n)


def sumsq_loops(n, grid):
    """Which loops of sumsq_kernel run at (n, grid workgroups of 256): (threads entering the unrolled loop, most unrolled trips
    of a thread, threads entering the remainder loop, most remainder trips of a thread) -- the launch arithmetic restated."""
    n4, stride = n // 4, grid * 256
    i = np.arange(stride, dtype=np.int64)
    trips = np.where(i + 3 * stride < n4, (n4 - 3 * stride - i + 4 * stride - 1) // (4 * stride), 0)
    rest = i + trips * 4 * stride
    rem = np.where(rest < n4, (n4 - rest + stride - 1) // stride, 0)
    return int((trips > 0).sum()), int(trips.max()), int((rem > 0).sum()), int(rem.max())


def sumsq_grid(n, cap=256):
    return min((n // 4 + 255) // 256 + 1, cap)


ADAM_N = (1, 255, 100003, 1048576 + 257)
ADAM_WD = (0.0, 0.01)
ADAM_CLIP = ("active", "inactive", "null", "zero")
ADAM_HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)
ADAM_BIG_STEP = 100000


def adam_inputs(n):
    g = torch.Generator().manual_seed(5000 + n % 9973)
    p = torch.randn(n, generator=g)
    grad = torch.randn(n, generator=g) * 3
    if n == 1:
        grad = grad.abs() + 1.0
    return p, grad


def adam_clip(kind, grad):
    """(gnorm_sq as the float32 the kernel reads, or None; max_norm) of a clip state"""
    q = f32(sumsq(grad))
    norm = math.sqrt(q)
    if kind == "active":
        return q, f32(norm / 50)
    if kind == "inactive":
        return q, f32(norm * 10)
    if kind == "null":
        return None, 1.0
    return q, 0.0


WSUM_CASES = (            # (n, widx)
    (1, (-1,)),
    (3, (15, -1, 15)),
    (16, (0, 1, 2, 3, -1, 5, 5, 5, 15, 9, 10, -1, 12, 0, 14, 15)),
)


def wsum_inputs(n):
    g = torch.Generator().manual_seed(6000 + n)
    return torch.randn(n, generator=g) * 2, torch.rand(16, generator=g) * 3 + 0.25          # distinct terms, the 16 weights


INFONCE_B = (2, 3, 7, 33, 64)
INFONCE_D = (64, 100, 256, 512)
INFONCE_T = (0.1, 0.5)
INFONCE_LAYOUTS = ("balanced", "singleton", "one-class", "distinct")


def labels(layout, B):
    if layout == "balanced":
        return torch.cat([torch.zeros(B // 2, dtype=torch.long), torch.ones(B - B // 2, dtype=torch.long)])
    if layout == "singleton":             # row 0 alone in its class; B = 2 leaves no room for partners elsewhere: both rows are singletons
        rest = B - 1
        other = [1] * rest if rest < 4 else [1] * (rest // 2) + [2] * (rest - rest // 2)
        return torch.tensor([0] + other, dtype=torch.long)
    if layout == "one-class":
        return torch.zeros(B, dtype=torch.long)
    return torch.arange(B, dtype=torch.long)


def embeddings(B, D, seed=0):
    g = torch.Generator().manual_seed(7000 + 131 * B + D + 100003 * seed)
    return torch.randn(B, D, generator=g), torch.randn(B, D, generator=g)


# HSIC: (name, B, D, layout, seed).  "plain": style and content ~ N(0, 1), a seed that meets the median condition.  Among the
# 2B^2 - B distinct pairs of 2B such rows the distances near the median lie ~ 4 / (2B^2) apart, so from B = 33 on hardly any seed
# leaves the 1e-4 relative gap (none of 200 at B = 33); "apart" adds 40 to every content coordinate instead.  That changes neither kernel matrix (both see only
# differences within style or within content) but moves all B^2 style-content distances above the B^2 - B others, so the lower
# median is the LARGEST within-group distance, which is isolated for most seeds.  "near": content = style + 0.05 * noise.
HSIC_CASES = (
    ("B2-D100", 2, 100, "plain", 0), ("B2-D256", 2, 256, "plain", 0),
    ("B3-D100", 3, 100, "plain", 0), ("B3-D256", 3, 256, "plain", 0),
    ("B7-D100", 7, 100, "plain", 0), ("B7-D256", 7, 256, "plain", 0),
    ("B33-D100", 33, 100, "apart", 0), ("B33-D256", 33, 256, "apart", 0),
    ("B64-D100", 64, 100, "apart", 0), ("B64-D256", 64, 256, "apart", 0),
    ("B128-D100", 128, 100, "apart", 0), ("B128-D256", 128, 256, "apart", 0),
    ("near-B7-D256", 7, 256, "near", 3),
)
HSIC_GAP = 1e-4


def hsic_inputs(B, D, layout, seed):
    s, c = embeddings(B, D, seed)
    if layout == "apart":
        c = c + 40.0
    elif layout == "near":
        c = s + 0.05 * c
    return s, c


CROSSCOV_B = (2, 3, 7, 33, 64, 256)
EMB_D = (100, 256)

MARGIN_CASES = tuple((C, D) for C in (2, 3, 5) for D in (100, 256))
MARGIN = 2.0


def margin_rows(C, D):
    """Class means for margin 2: `inside` lies 1 from row 0, `outside` 5 from it, `far` is an independent N(0, 1) row."""
    g = torch.Generator().manual_seed(8000 + 10 * C + D)
    r0, far = torch.randn(D, generator=g), torch.randn(D, generator=g)
    u, w = torch.randn(D, generator=g), torch.randn(D, generator=g)
    inside, outside = r0 + u / u.norm(), r0 + 5 * w / w.norm()
    rows = {(2, 100): [r0, inside],                        # one pair, inside the margin
            (2, 256): [r0, outside],                       # one pair, outside: the gradient is exactly 0
            (3, 100): [r0, inside, outside],
            (3, 256): [r0, r0, inside],                    # identical rows: dist = 0, the guarded branch
            (5, 100): [r0, inside, outside, outside, far],
            (5, 256): [r0, inside, outside, far, r0]}[(C, D)]
    return torch.stack(rows).clone()


def margin_pairs(cls, m=MARGIN):
    """(pairs inside the margin at dist > 0, pairs outside, pairs at dist == 0) in float64"""
    d = torch.pdist(cls.double())
    return int(((d < m) & (d > 0)).sum()), int((d >= m).sum()), int((d == 0).sum())


ROW_R = (1, 5, 257)
ROW_C = (1, 2, 7)
ROW_SCALE = (1.0, 50.0)


def row_inputs(R, C, scale_):
    g = torch.Generator().manual_seed(9000 + 10 * R + C)
    z = torch.randn(R, C, generator=g) * scale_
    t = torch.randint(0, C, (R,), generator=g, dtype=torch.int32)
    t[0], t[-1] = 0, C - 1                               # R == 1: the one target is C - 1
    if R >= 3:
        t[1] = C - 1
    return z, t


SCALE_N = (1, 1048576 + 5)

# (name, B, S, T, Fq, row stride of the target, phases)
RECON_CASES = (
    ("real-size", 2, 2, 287, 513, 513, "random"),        # 294462 bins > 256 workgroups x 1024: threads stride, workgroups share slots
    ("one-bin", 1, 1, 1, 1, 1, "random"),
    ("one-row", 3, 1, 1, 7, 7, "random"),                # no neighbour in section or in time
    ("one-column", 1, 3, 5, 1, 1, "random"),             # no neighbour in frequency
    ("padded-target", 2, 3, 5, 9, 16, "random"),         # tgt_ld = Fq + 7
    ("branch-cut", 2, 2, 6, 11, 11, "cut"),              # out near +pi - 0.05 against tgt near -pi + 0.05, and the reverse
)
RECON_MIN_MAG = 0.05
RECON_PHASE_GUARD = 0.02


def recon_inputs(B, S, T, Fq, ld, phases, seed=0):
    """(out (B,S,2,T,Fq), x (B,S,2,T,ld)) float32, the target x[..., :Fq].  Magnitudes |N(0,1)| + 0.06.  "random": target phase
    uniform, the wrapped difference uniform in +-(pi - 0.05), so the raw difference of the two atan2 crosses the branch cut in
    about half of the bins.  "cut": every bin sits at the cut, even bins one way round and odd bins the other."""
    g = np.random.default_rng([11000 + seed, B, S, T, Fq])
    shape = (B, S, T, Fq)
    mag_o, mag_t = np.abs(g.standard_normal(shape)) + 0.06, np.abs(g.standard_normal(shape)) + 0.06
    if phases == "cut":
        jit = g.uniform(-0.02, 0.02, (2,) + shape)
        odd = (np.arange(np.prod(shape)).reshape(shape) % 2).astype(bool)
        ph_o = np.where(odd, -np.pi + 0.05, np.pi - 0.05) + jit[0]
        ph_t = np.where(odd, np.pi - 0.05, -np.pi + 0.05) + jit[1]
    else:
        ph_t = g.uniform(-np.pi, np.pi, shape)
        ph_o = ph_t + g.uniform(-np.pi + 0.05, np.pi - 0.05, shape)
    out = np.stack([mag_o * np.cos(ph_o), mag_o * np.sin(ph_o)], axis=2).astype(np.float32)
    x = (0.5 * g.standard_normal((B, S, 2, T, ld))).astype(np.float32)
    x[..., :Fq] = np.stack([mag_t * np.cos(ph_t), mag_t * np.sin(ph_t)], axis=2).astype(np.float32)
    return torch.from_numpy(out), torch.from_numpy(x)


def wrapped_phase_difference(out, tgt):
    d = torch.atan2(out[:, :, 1].double(), out[:, :, 0].double()) - torch.atan2(tgt[:, :, 1].double(), tgt[:, :, 0].double())
    return torch.remainder(d + math.pi, 2 * math.pi) - math.pi
