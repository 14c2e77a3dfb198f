"""Float64 references of the normalisation kernels of csrc/norm.hip, written as formulas, plus the case tables, seeded inputs,
bounds and launch arithmetic that tests/test_norm_cpu.py (no GPU) and tests/test_gpu_norm.py share: the channel statistics, the
finalize, apply and backward passes of BatchNorm2d / InstanceNorm2d (relu?(BN(x) [+ IN(r)]), the ResBlock tail), their
fused-finalize twins, LayerNorm and the fused residual + dropout + LayerNorm.

Activations are NHWC, here (N, HW, C).  Channels >= Creal are padding: gamma and beta have Creal entries, the kernels give such a
channel scale = shift = 0 whatever it holds, and the references do the same by padding gamma and beta with zeros.

Tolerances are measured, never chosen (`bound`, the rule of tests/loss_tail_ref.py extended by conditioning): e32 = the error of the
plain float32 evaluation (torch's batch norm / layer norm and float32 autograd) against float64 on the same inputs, relative to
max |float64|, and a kernel must be within max(8 * e32, 64 * 2^-24 * max(1, kappa / 4)).  kappa = 1 + max over channels of
(mean / std)^2 from the float64 reference: the kernels form the variance as E[x^2] - m^2 and the backward's S1 - m * S0 from float32
sums (the table format the GEMM epilogues share), which loses kappa * 2^-24, where torch's Welford does not.  kappa applies to what
depends on a variance or on S1 - m * S0; plain sums, dbeta and the LayerNorm kernels (two-pass variance) get kappa = 1, and while
kappa / 4 <= 1 the bound is loss_tail_ref's.  A constant channel (variance exactly 0) is exact by construction and does not count towards
kappa.  A bf16 tensor that a kernel stores gets 2^-8 more: one bf16 rounding (half an ulp is 2^-9), doubled.

Where ReLU is on, every pre-activation of a real channel is at least MARGIN * max |pre| away from 0 in the float64 reference, nothing
excluded, so no mask bit that rounding could flip decides a comparison.  No seed gives that at these sizes (3e-3 of a random draw lies
inside the margin), so `bn_inputs` MOVES the offending x away from it and re-derives the statistics: at most 1.3 % of the elements, in
one pass, separately for every variant a test runs (BN(x) alone and BN(x) + IN(r) have different pre-activations, hence
different x).  tests/test_norm_cpu.py asserts the margin, and that float32 takes the same mask, for every variant of gpu_variants()."""
from __future__ import annotations

import functools
import os

import numpy as np
import torch

U24 = 2.0 ** -24
FLOOR = 64 * U24
FACTOR = 8.0
BF16_STORE = 2.0 ** -8
F64 = torch.float64
MARGIN = 1e-3
MOMENTUM = 0.1
EPS = 1e-5


def rel(a, ref):
    """max |a - ref| / max |ref| in float64"""
    a, ref = torch.as_tensor(a).detach().double().cpu().reshape(-1), torch.as_tensor(ref).detach().double().cpu().reshape(-1)
    return float((a - ref).abs().max() / max(float(ref.abs().max()), 1e-300))


def bound(plain32, ref64, kappa=1.0, bf16_store=False):
    """(e32, tolerance) for one compared quantity"""
    e32 = rel(plain32, ref64)
    return e32, max(FACTOR * e32, FLOOR * max(1.0, kappa / 4.0)) + (BF16_STORE if bf16_store else 0.0)


def is_zero(ref):
    return float(torch.as_tensor(ref).abs().max()) == 0.0


def rounded(t, dtype):
    """t rounded to dtype, as float64: the values a kernel of that dtype sees"""
    return t.to(dtype).double()


# ---- launch arithmetic of csrc/norm.hip, restated ----------------------------------------------------------------------------

def _env_int(name, fallback):
    e = os.environ.get(name)
    try:
        return int(e) if e is not None else fallback
    except ValueError:
        return 0                                            # atoi of a non-number


def reduce_blocks():
    return _env_int("AST_REDUCE_BLOCKS", 512)


def elem_blocks():
    return _env_int("AST_ELEM_BLOCKS", 2048)


def _cdiv(a, b):
    return (a + b - 1) // b


def reduce_launch(N, HW, C, nslots=None):
    """ast_chan_stats / ast_norm_bwd_sums[_pre] (nslots None) and their _det forms: the grid and what its workgroups do."""
    U = C // 8
    PL = 256 // U
    if nslots is None:
        nblk = max(1, min(_cdiv(HW, PL), max(1, reduce_blocks() // N)))
        ppb = _cdiv(HW, nblk)
        gx = _cdiv(HW, ppb)
    else:
        ppb, gx = _cdiv(HW, nslots), nslots
    pix = [max(0, min(HW, (b + 1) * ppb) - b * ppb) for b in range(gx)]
    return dict(U=U, PL=PL, ppb=ppb, grid=(gx, N), idle_threads=256 - PL * U, lanes_without_pixel=min(pix) < PL,
                ragged_last_block=gx > 1 and 0 < pix[-1] < ppb, empty_slots=sum(1 for p in pix if p == 0),
                one_workgroup_per_image=gx == 1 and N > reduce_blocks())


def elem_launch(N, HW, C):
    """ast_affine_act / ast_norm_bwd_apply[_pre] / ast_bn_apply_fwd / _bwd: grid = (blocks per image, N) of 256 threads, a thread
    takes `trips` 8-channel units of its image; hoist: the unit's coefficients are loaded once, before the loop."""
    U = C // 8
    per_img = HW * U
    gx = max(1, min(_cdiv(per_img, 256), max(1, elem_blocks() // N)))
    return dict(U=U, grid=(gx, N), trips=_cdiv(per_img, gx * 256), hoist=256 % U == 0)


def apply_launch(rows, C, backward=False):
    """the slot reduction at the head of ast_bn_apply_fwd / _bwd: threads per channel and dynamic LDS bytes; accepted: rows * C <= 65536"""
    nparts = max(1, min(rows, 256 // min(C, 256)))
    return dict(nparts=nparts, lds=4 * ((6 if backward else 4) * C + 2 * C * nparts), accepted=rows * C <= 65536)


# ---- float64 references --------------------------------------------------------------------------------------------------------

def chan_sums(x):
    """{sum x, sum x^2} per image and channel: (N, C, 2)"""
    return torch.stack([x.sum(1), (x * x).sum(1)], -1)


def pad_params(p, C):
    out = torch.zeros(C, dtype=p.dtype)
    out[:p.numel()] = p
    return out


def moments(x, dims):
    m = x.mean(dims, keepdim=True)
    return m.squeeze(dims), ((x - m) ** 2).mean(dims)


def kappa_of(mean, var):
    """1 + max (mean / std)^2 over the statistics with a variance (a constant channel is exact by construction)"""
    live = var > 0
    if not bool(live.any()):
        return 1.0
    return 1.0 + float((mean[live] ** 2 / var[live]).max())


def finalize(mean, var, gamma, beta, eps):
    """(rstd, scale, shift); gamma / beta already padded to the statistics' channel count (broadcast over leading dims)"""
    rstd = (var + eps) ** -0.5
    scale = gamma * rstd
    return rstd, scale, beta - mean * scale


def running_update(rm, rv, mean, var, cnt, Creal):
    """nn.BatchNorm2d's update: momentum 0.1, the unbiased variance var * cnt / max(cnt - 1, 1)"""
    return ((1 - MOMENTUM) * rm + MOMENTUM * mean[:Creal], (1 - MOMENTUM) * rv + MOMENTUM * var[:Creal] * cnt / max(cnt - 1, 1))


def bwd_coefs(S0, S1, mean, rstd, gamma, P):
    """Q = rstd (S1 - m S0) (the gamma gradient), and k[..., 3] with dx = k0 dz + k1 x + k2"""
    Q = rstd * (S1 - mean * S0)
    k = torch.stack([gamma * rstd, -gamma * rstd * rstd * Q / P, -gamma * rstd * S0 / P + gamma * rstd * rstd * mean * Q / P], -1)
    return Q, k


def bn_forward_backward(x, r, g1, b1, g2, b2, relu, dy, eps1=EPS, eps2=EPS, dtype=F64):
    """relu?(BN(x) [+ IN(r)]) and its whole backward, by formulas, in `dtype`.  x, r, dy: (N, HW, C); g1, b1 (g2, b2): Creal
    entries.  Every intermediate a kernel writes is returned."""
    x, dy = x.to(dtype), dy.to(dtype)
    N, HW, C = x.shape
    Creal = g1.numel()
    G1, B1 = pad_params(g1.to(dtype), C), pad_params(b1.to(dtype), C)
    o = {"sums1": chan_sums(x)}
    m1, v1 = moments(x, (0, 1))
    rs1, sc1, sf1 = finalize(m1, v1, G1, B1, eps1)
    o.update(mean1=m1, var1=v1, rstd1=rs1, scale1=sc1, shift1=sf1, kappa1=kappa_of(m1, v1))
    pre = x * sc1 + sf1
    if r is not None:
        r = r.to(dtype)
        G2, B2 = pad_params(g2.to(dtype), C), pad_params(b2.to(dtype), C)
        o["sums2"] = chan_sums(r)
        m2, v2 = moments(r, (1,))                                                          # (N, C)
        rs2, sc2, sf2 = finalize(m2, v2, G2, B2, eps2)
        o.update(mean2=m2, var2=v2, rstd2=rs2, scale2=sc2, shift2=sf2, kappa2=kappa_of(m2, v2))
        pre = pre + (r * sc2[:, None] + sf2[:, None])
    o["pre"] = pre
    o["y"] = pre.clamp(min=0) if relu else pre
    dz = torch.where(pre > 0, dy, torch.zeros_like(dy)) if relu else dy
    o["relu_bwd"] = dz                                                                     # ast_norm_bwd_apply with k1 = NULL
    S0, S1 = dz.sum(1), (dz * x).sum(1)                                                    # (N, C)
    S2 = (dz * r).sum(1) if r is not None else torch.zeros_like(S0)
    o["sums3"] = torch.stack([S0, S1, S2], -1)
    Q1, k1 = bwd_coefs(S0.sum(0), S1.sum(0), m1, rs1, G1, N * HW)
    o.update(k1=k1, dgamma1=Q1[:Creal], dbeta1=S0.sum(0)[:Creal])
    o["dx"] = k1[:, 0] * dz + k1[:, 1] * x + k1[:, 2]
    if r is not None:
        Q2, k2 = bwd_coefs(S0, S2, m2, rs2, G2, HW)
        o.update(k2=k2, dgamma2=Q2.sum(0)[:Creal], dbeta2=S0.sum(0)[:Creal])
        o["dr"] = k2[:, None, :, 0] * dz + k2[:, None, :, 1] * r + k2[:, None, :, 2]
    return o


def bn_plain32(x, r, g1, b1, g2, b2, relu, dy, rm, rv, eps1=EPS, eps2=EPS):
    """The same quantities from torch in float32: native batch norm (Welford statistics) for both branches, float32 autograd for the
    gradients; the sums and the k coefficients, which torch never forms, by the formulas in float32 from torch's statistics."""
    f = torch.float32
    N, HW, C = x.shape
    Creal = g1.numel()
    x32, dy32 = x.to(f).requires_grad_(True), dy.to(f)
    G1, B1 = pad_params(g1.to(f), C).requires_grad_(True), pad_params(b1.to(f), C).requires_grad_(True)
    rm32, rv32 = pad_params(rm.to(f), C), pad_params(rv.to(f), C)
    rv32[Creal:] = 1.0
    xc = x32.permute(0, 2, 1)                                                              # (N, C, HW)
    ybn, m1, rs1 = torch.native_batch_norm(xc, G1, B1, rm32, rv32, True, MOMENTUM, eps1)
    o = {"sums1": chan_sums(x32.detach()), "mean1": m1.detach(), "rstd1": rs1.detach(), "scale1": (G1 * rs1).detach(),
         "shift1": (B1 - m1 * G1 * rs1).detach(), "running_mean": rm32[:Creal], "running_var": rv32[:Creal]}
    pre = ybn
    leaves = [x32, G1, B1]
    if r is not None:
        r32 = r.to(f).requires_grad_(True)
        G2, B2 = pad_params(g2.to(f), C).requires_grad_(True), pad_params(b2.to(f), C).requires_grad_(True)
        rc = r32.permute(0, 2, 1).reshape(1, N * C, HW)
        yin, m2, rs2 = torch.native_batch_norm(rc, G2.repeat(N), B2.repeat(N), None, None, True, MOMENTUM, eps2)
        m2, rs2 = m2.view(N, C), rs2.view(N, C)
        pre = pre + yin.view(N, C, HW)
        o.update(sums2=chan_sums(r32.detach()), mean2=m2.detach(), rstd2=rs2.detach(), scale2=(G2 * rs2).detach(),
                 shift2=(B2 - m2 * G2 * rs2).detach())
        leaves += [r32, G2, B2]
    y = (torch.relu(pre) if relu else pre).permute(0, 2, 1)
    o["pre"], o["y"] = pre.detach().permute(0, 2, 1), y.detach()
    grads = torch.autograd.grad(y, leaves, dy32)
    o.update(dx=grads[0], dgamma1=grads[1][:Creal], dbeta1=grads[2][:Creal])
    with torch.no_grad():
        dz = torch.where(o["pre"] > 0, dy32, torch.zeros_like(dy32)) if relu else dy32
        o["relu_bwd"] = dz
        xd = x32.detach()
        S0, S1 = dz.sum(1), (dz * xd).sum(1)
        S2 = (dz * r32.detach()).sum(1) if r is not None else torch.zeros_like(S0)
        o["sums3"] = torch.stack([S0, S1, S2], -1)
        o["k1"] = bwd_coefs(S0.sum(0), S1.sum(0), o["mean1"], o["rstd1"], G1.detach(), N * HW)[1]
        if r is not None:
            o.update(dr=grads[3], dgamma2=grads[4][:Creal], dbeta2=grads[5][:Creal])
            o["k2"] = bwd_coefs(S0, S2, o["mean2"], o["rstd2"], G2.detach(), HW)[1]
    return o


def layernorm(x, gamma, beta, eps=EPS):
    """(y, mean, rstd) over the last dim"""
    m, v = moments(x, (-1,))
    rstd = (v + eps) ** -0.5
    return (x - m[..., None]) * rstd[..., None] * gamma + beta, m, rstd


def layernorm_bwd(dy, x, gamma, mean, rstd):
    """(dx, dgamma, dbeta): g = dy gamma, dx = rstd (g - mean(g) - xh mean(g xh))"""
    xh = (x - mean[..., None]) * rstd[..., None]
    g = dy * gamma
    dx = rstd[..., None] * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    return dx, (dy * xh).sum(0), dy.sum(0)


def add_drop_ln(x, sub, mask, gamma, beta, eps=EPS):
    """s = x + mask * sub (x, mask may be None); (s, y, mean, rstd), the last three None without gamma"""
    s = sub * mask if mask is not None else sub.clone()
    if x is not None:
        s = s + x
    if gamma is None:
        return s, None, None, None
    return (s,) + layernorm(s, gamma, beta, eps)


def add_drop_ln_bwd(dy, ds_ext, s, gamma, mean, rstd, mask):
    """ds = ds_ext + LN_bwd(dy; s) (either may be None); -> (dx = ds, dsub = ds * mask, dgamma, dbeta)"""
    ds = torch.zeros_like(s) if ds_ext is None else ds_ext.clone()
    dg = db = None
    if dy is not None:
        d, dg, db = layernorm_bwd(dy, s, gamma, mean, rstd)
        ds = ds + d
    return ds, ds * mask if mask is not None else ds, dg, db


# ---- BatchNorm / InstanceNorm cases and seeded inputs ------------------------------------------------------------------------------

# name: (N, HW, C, Creal, mean/std of x, second (InstanceNorm) input?, constant channel or None, dtypes)
BOTH, F32_ONLY = (torch.float32, torch.bfloat16), (torch.float32,)
BN_CASES = {
    "c8-pad":      (3, 117, 8, 2, 0, True, None, BOTH),          # U = 1, PL = 256 > HW: lanes without a pixel; 6 padded channels
    "c24":         (3, 117, 24, 24, 0, True, None, BOTH),        # 256 % 3 != 0: per-iteration coefficients, one idle thread, ragged last block
    "c24-r8":      (3, 117, 24, 24, 8, True, None, BOTH),
    "c40-r2":      (1, 1600, 40, 40, 2, True, None, BOTH),       # 256 % 5 != 0, 32 workgroups per image
    "c64-r32":     (3, 117, 64, 64, 32, True, None, BOTH),
    "c256":        (1, 3, 256, 256, 0, False, None, BOTH),       # nparts = 1; PL = 8 > HW
    "c512-const":  (3, 20, 512, 512, 0, False, 5, BOTH),         # channel 5 holds 0.5 everywhere: var = 0, rstd = eps^-1/2
    "c2048":       (1, 3, 2048, 2048, 0, False, None, BOTH),     # U = 256, PL = 1
    "hw1":         (3, 1, 64, 64, 0, False, None, BOTH),
    "many-images": (600, 3, 8, 8, 0, False, None, BOTH),         # N > reduce_blocks(): one workgroup per image; finalize lanes loop over N
    "stride2":     (256, 300, 64, 64, 0, True, None, F32_ONLY),  # elem_blocks() / N = 8 workgroups per image: a second grid-stride trip
}
BN_IDS = [f"{n}-{'f32' if d == torch.float32 else 'bf16'}" for n, c in BN_CASES.items() for d in c[7]]
BN_PARAMS = [(n, d) for n, c in BN_CASES.items() for d in c[7]]

# the path every named case is claimed to enter (tests/test_norm_cpu.py checks each claim against the launch arithmetic, and that
# no path is left without a case)
PATH_CLAIMS = {
    "hoist-off":               ("c24", "c24-r8", "c40-r2"),
    "PL=1":                    ("c2048",),
    "PL=256":                  ("c8-pad", "many-images"),
    "idle-threads":            ("c24", "c40-r2"),
    "lanes-without-pixel":     ("c8-pad", "c256", "hw1"),
    "ragged-last-block":       ("c24", "c24-r8"),
    "one-workgroup-per-image": ("many-images",),
    "second-grid-stride-trip": ("stride2",),
    "constant-channel":        ("c512-const",),
    "padded-channels":         ("c8-pad",),
    "ratio-0":                 ("c24",),
    "ratio-2":                 ("c40-r2",),
    "ratio-8":                 ("c24-r8",),
    "ratio-32":                ("c64-r32",),
}
PATH_TESTS = {
    "hoist-off":               lambda c, red, el: not el["hoist"],
    "PL=1":                    lambda c, red, el: red["PL"] == 1,
    "PL=256":                  lambda c, red, el: red["PL"] == 256,
    "idle-threads":            lambda c, red, el: red["idle_threads"] > 0,
    "lanes-without-pixel":     lambda c, red, el: red["lanes_without_pixel"],
    "ragged-last-block":       lambda c, red, el: red["ragged_last_block"],
    "one-workgroup-per-image": lambda c, red, el: red["one_workgroup_per_image"],
    "second-grid-stride-trip": lambda c, red, el: el["trips"] >= 2,
    "constant-channel":        lambda c, red, el: c[6] is not None,
    "padded-channels":         lambda c, red, el: c[3] < c[2],
    "ratio-0":                 lambda c, red, el: c[4] == 0,
    "ratio-2":                 lambda c, red, el: c[4] == 2,
    "ratio-8":                 lambda c, red, el: c[4] == 8,
    "ratio-32":                lambda c, red, el: c[4] == 32,
}

DET_SLOTS = (1, 3, 64)                                      # ast_chan_stats_det / ast_norm_bwd_sums_det; 64 > HW in DET_CASES[0]
DET_CASES = ("hw3-det", "c24")                              # hw3-det: HW = 3 < 64 slots: 61 slots per image without a pixel
BN_CASES_EXTRA = {"hw3-det": (3, 3, 24, 24, 0, False, None, BOTH)}

# slot tables with the pixel count passed separately: (rows, case whose pixels are dealt into the rows) -> nparts 1, 8, 10, 32,
# and the largest table accepted (32 x 2048)
SLOT_CASES = ((1, "c64-r32"), (8, "c24"), (16, "c24-r8"), (64, "c8-pad"), (32, "c2048"))
SLOT_REJECTED = (33, "c2048")                               # rows * C = 65536 + C


AUTOGRAD_CASES = ("c24", "c24-r8")                         # AL.bn_act and ops.ResTailFn: C = 24 and mean / std = 8
ONE_VARIANT = ("stride2",)    # 4.9 M elements per tensor: only relu(BN(x) + IN(r)), which keeps its tests at a few seconds


def variants(name):
    """the with-InstanceNorm-input flags a case is run at"""
    if not case(name)[5]:
        return (False,)
    return (True,) if name in ONE_VARIANT else (False, True)


def case(name):
    return BN_CASES[name] if name in BN_CASES else BN_CASES_EXTRA[name]


def _seed(name):
    return 20000 + sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % 9973


def _pre_of(x, r, p):
    o = {}
    N, HW, C = x.shape
    G1, B1 = pad_params(p["g1"], C), pad_params(p["b1"], C)
    m1, v1 = moments(x, (0, 1))
    _, sc1, sf1 = finalize(m1, v1, G1, B1, EPS)
    pre = x * sc1 + sf1
    if r is not None:
        m2, v2 = moments(r, (1,))
        _, sc2, sf2 = finalize(m2, v2, pad_params(p["g2"], C), pad_params(p["b2"], C), EPS)
        pre = pre + r * sc2[:, None] + sf2[:, None]
    return pre, sc1


def relu_margin(pre, Creal):
    """min |pre| / max |pre| over the real channels"""
    q = pre[..., :Creal].abs()
    return float(q.min() / q.max())


@functools.lru_cache(maxsize=None)
def bn_inputs(name, dtype, relu=True, with_r=True):
    """Seeded inputs of one variant of a case, every activation already rounded to `dtype` and held as float64.
      x      per-channel std in [0.5, 2], mean = ratio * std with alternating sign; with at most 8 pixels per channel the values are
             spread evenly plus a little noise, so that no channel's sample mean / std is huge by chance
      r      3 N(0, 1) + 1, or None: the case has no second input, or this is its BatchNorm-only variant (with_r False)
      dy     N(0, 1)
      gamma  in [0.5, 1.5];  |beta| >= 0.1;  running_mean ~ 0.1 N(0, 1), running_var in [0.5, 1.5]
    With relu, x is then MOVED, not reseeded: about 3e-3 of the pre-activations of a random draw lie within MARGIN of zero, thousands
    of elements per case, so no seed meets the condition by itself.  Every x whose pre-activation (of THIS variant: BN(x) alone or
    BN(x) + IN(r)) lies within 2 * MARGIN * max |pre| of 0 in a real channel is stepped away from it, by at least 8 * MARGIN * max
    |pre| in pre and at least 2^-6 |x|; the statistics are re-derived, and this repeats until nothing lies within MARGIN.  The
    constant channel is never touched (its pre-activation is beta).  `moved` is the number of elements that differ from the draw,
    `rounds` the number of passes: 0 ... 1.3 % of the real-channel elements, in one pass (test_norm_cpu.py prints and bounds them)."""
    N, HW, C, Creal, ratio, has_r, const, _ = case(name)
    with_r = bool(with_r and has_r)
    g = torch.Generator().manual_seed(_seed(name))
    std = torch.rand(C, generator=g, dtype=F64) * 1.5 + 0.5
    sign = torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0).double()
    x = torch.randn(N, HW, C, generator=g, dtype=F64)
    if N * HW <= 8:
        spread = torch.linspace(-1.5, 1.5, N * HW, dtype=F64).reshape(N, HW, 1)
        x = 0.2 * x + spread * torch.where(torch.arange(C) % 3 == 0, -1.0, 1.0).double()
    x = x * std + ratio * std * sign
    if const is not None:
        x[..., const] = 0.5
    r = torch.randn(N, HW, C, generator=g, dtype=F64) * 3 + 1 if has_r else None          # drawn for both variants: the same x and dy
    dy = torch.randn(N, HW, C, generator=g, dtype=F64)
    p = {}
    for k in ("1", "2"):
        p["g" + k] = torch.rand(Creal, generator=g, dtype=F64) + 0.5
        b = torch.randn(Creal, generator=g, dtype=F64) * 0.2
        p["b" + k] = torch.where(b >= 0, b + 0.1, b - 0.1)
    p["rm"] = torch.randn(Creal, generator=g, dtype=F64) * 0.1
    p["rv"] = torch.rand(Creal, generator=g, dtype=F64) + 0.5
    p = {k: rounded(v, torch.float32) for k, v in p.items()}                               # parameters are float32 in every mode
    x, dy = rounded(x, dtype), rounded(dy, dtype)
    r = rounded(r, dtype) if with_r else None
    drawn, rounds = x, 0
    if relu:
        for rounds in range(200):
            pre, sc1 = _pre_of(x, r, p)
            thr = MARGIN * float(pre[..., :Creal].abs().max())
            if not bool((pre[..., :Creal].abs() < thr).any()):
                break
            near = pre.abs() < 2 * thr
            near[..., Creal:] = False
            if const is not None:
                near[..., const] = False
            away = torch.sign(pre) * torch.sign(sc1)
            away = torch.where(away == 0, torch.ones_like(away), away)
            step = away * torch.maximum(8 * thr / sc1.abs().clamp(min=1e-30), x.abs() * 2.0 ** -6)
            x = rounded(torch.where(near, x + step, x), dtype)
    return dict(x=x, r=r, dy=dy, N=N, HW=HW, C=C, Creal=Creal, const=const, moved=int((x != drawn).sum()), rounds=rounds, **p)


@functools.lru_cache(maxsize=None)
def bn_reference(name, dtype, relu=True, with_r=True):
    """(float64 reference, plain float32 evaluation, kappa) of one variant of a case, on that variant's own inputs"""
    i = bn_inputs(name, dtype, relu, with_r)
    r = i["r"]
    ref = bn_forward_backward(i["x"], r, i["g1"], i["b1"], i["g2"], i["b2"], relu, i["dy"])
    cnt = i["N"] * i["HW"]
    ref["running_mean"], ref["running_var"] = running_update(i["rm"], i["rv"], ref["mean1"], ref["var1"], cnt, i["Creal"])
    plain = bn_plain32(i["x"], r, i["g1"], i["b1"], i["g2"], i["b2"], relu, i["dy"], i["rm"], i["rv"])
    return ref, plain, max(ref["kappa1"], ref.get("kappa2", 1.0))


def gpu_variants():
    """Every (name, dtype, with_r) that tests/test_gpu_norm.py runs with ReLU on: the case table at its variants, the deterministic
    cases, the slot tables (float32, BatchNorm only) and the autograd cases."""
    out = [(n, d, w) for n, d in BN_PARAMS for w in variants(n)]
    out += [(n, d, bool(case(n)[5])) for n in DET_CASES for d in BOTH]
    out += [(n, torch.float32, False) for _, n in SLOT_CASES + (SLOT_REJECTED,)]
    out += [(n, d, w) for n in AUTOGRAD_CASES for d in BOTH for w in (False, True)]
    return sorted(set(out), key=lambda v: (v[0], str(v[1]), v[2]))


def slot_split(t, rows):
    """(N, HW, C) pixels dealt into `rows` contiguous groups -> list of (pixels, C) tensors, some possibly empty"""
    flat = t.reshape(-1, t.shape[-1])
    n = flat.shape[0]
    per = _cdiv(n, rows)
    return [flat[i * per:(i + 1) * per] for i in range(rows)]


# which quantities carry the conditioning of a variance or of S1 - m S0, and of which branch (the ReLU-masked dy, the plain sums, the
# means and dbeta carry none); and which a kernel stores in the activation dtype
KAPPA1_KEYS = {"rstd1", "scale1", "shift1", "running_var", "k1", "dgamma1", "dx"}
KAPPA2_KEYS = {"rstd2", "scale2", "shift2", "k2", "dgamma2", "dr"}
KAPPA_BOTH_KEYS = {"y", "pre"}
STORED_KEYS = {"y", "dx", "dr", "relu_bwd"}


def kappa_for(key, ref):
    """the kappa of norm_ref.bound for the reference quantity `key` of bn_forward_backward's result `ref`"""
    k1, k2 = ref["kappa1"], ref.get("kappa2", 1.0)
    return k1 if key in KAPPA1_KEYS else k2 if key in KAPPA2_KEYS else max(k1, k2) if key in KAPPA_BOTH_KEYS else 1.0


# ---- LayerNorm / add_drop_ln cases ---------------------------------------------------------------------------------------------

LN_D = (1, 63, 64, 65, 256, 1000)
LN_ROWS = (1, 4, 5, 67)
ADLN_ROWS = (1, 5, 67)                                      # the 256-wide backward runs with 3, 3 and 1 invalid waves in its last workgroup
# operand combinations of ast_add_drop_ln_fwd / _bwd: (name, x, gamma (LayerNorm), p, dy, ds_ext, dx)
ADLN_COMBOS = (
    ("full",        True,  True,  0.3, True,  True,  True),
    ("x-null",      False, True,  0.3, True,  True,  True),
    ("gamma-null",  True,  False, 0.3, False, True,  True),     # s only: no LayerNorm, so only ds_ext can come back
    ("dy-only",     True,  True,  0.3, True,  False, True),
    ("ds-only",     True,  True,  0.3, False, True,  True),
    ("mask-null",   True,  True,  0.0, True,  True,  True),     # p = 0: no mask is written or read
    ("dx-null",     True,  True,  0.3, True,  True,  False),
)
ADLN_SEED, ADLN_OFFSET = 0x5EED1234ABCD, 5


@functools.lru_cache(maxsize=None)
def ln_inputs(rows, D):
    """x ~ 2 N(0, 1) + 0.3 (mean / std well below 1), sub ~ 1.5 N(0, 1), gamma in [0.5, 1.5], beta ~ 0.2 N(0, 1), dy, ds_ext ~ N(0, 1),
    and non-zero starting values of the parameter gradients; all float32 values held as float64"""
    g = torch.Generator().manual_seed(30000 + 1009 * rows + D)
    o = dict(x=torch.randn(rows, D, generator=g) * 2 + 0.3, sub=torch.randn(rows, D, generator=g) * 1.5,
             gamma=torch.rand(D, generator=g) + 0.5, beta=torch.randn(D, generator=g) * 0.2, dy=torch.randn(rows, D, generator=g),
             ds_ext=torch.randn(rows, D, generator=g), dgamma0=torch.randn(D, generator=g), dbeta0=torch.randn(D, generator=g))
    return {k: v.double() for k, v in o.items()}
