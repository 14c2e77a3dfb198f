"""Reference of the weight bank (csrc/weights.hip: ast_weights_prepare_t, ast_weight_grads_flush_t / _det, ast_weight_grad_unpack)
for ONE weight, in numpy, with no GPU and no library: spectral-norm power iteration and sigma (torch nn/utils/spectral_norm.py:92-114,
eps 1e-12), W/sigma in the two packed layouts, and the flush of the packed gradient staging into the gradient of weight_orig,

    grad += (dW - <dW, W/sigma> u v^T) / sigma,        dW = sum of the staging replicas.

Everything works on the LOGICAL weight W[co][ci][tap] (`logical` reads it out of a strided master: conv [co][ci][tap], conv-transpose
[ci][co][tap], linear [co][ci]); column j of the Co x (Ci*KK) matrix of the power iteration is ci*KK + tap, as in torch's
weight.permute(dim, ...).reshape(Co, -1).

`chain` evaluates the whole thing twice over the same inputs:
  * np.float64 -- the reference the kernels are compared with (tests/test_weight_bank_cpu.py holds it to torch's spectral_norm in
    float64 at 1e-12);
  * np.float32 with every reduction a SEQUENTIAL float32 sum (np.cumsum(..., dtype=float32)[-1]) and every elementwise step rounded
    to float32 -- not a model of the kernels, only a yardstick: its distance from the float64 result (`e_seq`) says how much float32
    arithmetic of this length, on these numbers, loses.  `bound_rel` turns it into the tolerance."""
from __future__ import annotations

import numpy as np

EPS = 1e-12
U24 = 2.0 ** -24
F32_CEILING = 2e-4            # the project's f32 op tolerance (tests/test_gpu_ops.py): no bound here may exceed it
BF16_ULP = 2.0 ** -8


def pad8(n):
    return (n + 7) // 8 * 8


def logical(storage, Co, Ci, KK, s_co, s_ci, offset=0):
    """W[co][ci][tap] = storage[offset + co*s_co + ci*s_ci + tap] as a (Co, Ci, KK) copy."""
    storage = np.ascontiguousarray(storage).reshape(-1)
    it = storage.itemsize
    return np.lib.stride_tricks.as_strided(storage[offset:], (Co, Ci, KK), (s_co * it, s_ci * it, it)).copy()


def scatter(storage, A, s_co, s_ci, offset=0):
    """The inverse of `logical`: write A[co][ci][tap] into a copy of the flat master `storage`."""
    out = np.array(storage).reshape(-1).copy()
    Co, Ci, KK = A.shape
    it = out.itemsize
    np.lib.stride_tricks.as_strided(out[offset:], (Co, Ci, KK), (s_co * it, s_ci * it, it))[...] = A
    return out


# ---- the two arithmetics ----------------------------------------------------------------------------------------------

def _sum(x, dt, axis=None):
    """float64: numpy's sum.  float32: the sequential left-to-right float32 sum."""
    if axis is None:
        x, axis = x.reshape(-1), 0
    if dt is np.float64:
        return x.sum(axis=axis, dtype=np.float64)
    assert x.dtype == np.float32
    return np.take(np.cumsum(x, axis=axis, dtype=np.float32), -1, axis=axis)


def _normalize(x, dt):
    """x / max(|x|_2, eps): torch.nn.functional.normalize(x, dim=0, eps=1e-12)"""
    n = np.sqrt(_sum(x * x, dt)).astype(dt)
    return (x / np.maximum(n, dt(EPS))).astype(dt)


def spectral(W, u, v, power_iter, dt=np.float64):
    """(u', v', sigma) of the (Co, Ci, KK) weight: one power iteration when power_iter, else u and v as given.
    u is None (no spectral norm): (None, None, 1)."""
    if u is None:
        return None, None, dt(1.0)
    Wm = W.reshape(W.shape[0], -1).astype(dt)
    u, v = u.astype(dt), v.astype(dt)
    if power_iter:
        v = _normalize(_sum(Wm * u[:, None], dt, axis=0).astype(dt), dt)       # W^T u
        u = _normalize(_sum(Wm * v[None, :], dt, axis=1).astype(dt), dt)       # W v
    Wv = _sum(Wm * v[None, :], dt, axis=1).astype(dt)
    sigma = dt(_sum(u * Wv, dt))
    return u, v, sigma


def pack(W, sigma, Cop, Cip, dt=np.float64):
    """wf[Cop][KK][Cip] and wb[Cip][KK][Cop] of W/sigma, zero in the padding."""
    Co, Ci, KK = W.shape
    Wn = (W.astype(dt) / dt(sigma)).astype(dt)
    wf = np.zeros((Cop, KK, Cip), dt)
    wf[:Co, :, :Ci] = Wn.transpose(0, 2, 1)
    wb = np.zeros((Cip, KK, Cop), dt)
    wb[:Ci, :, :Co] = Wn.transpose(1, 2, 0)
    return wf, wb


def stage(parts, from_wb, Cop, Cip, pad_value=0.0):
    """Physical gradient staging of the replicas parts[r][co][ci][tap]: (R, Cop*KK*Cip) float32, replica r in the [Cop][KK][Cip]
    (from_wb = 0) or [Cip][KK][Cop] (from_wb = 1) layout, the padding filled with pad_value."""
    R, Co, Ci, KK = parts.shape
    if from_wb:
        st = np.full((R, Cip, KK, Cop), pad_value, np.float32)
        st[:, :Ci, :, :Co] = parts.transpose(0, 2, 3, 1)
    else:
        st = np.full((R, Cop, KK, Cip), pad_value, np.float32)
        st[:, :Co, :, :Ci] = parts.transpose(0, 1, 3, 2)
    return st.reshape(R, -1)


def unstage(dwp, from_wb, R, Co, Ci, KK, Cop, Cip):
    """The valid part of a staging buffer as parts[r][co][ci][tap]; the padding is ignored."""
    dwp = np.asarray(dwp).reshape(-1)[:R * Cop * KK * Cip]
    if from_wb:
        return dwp.reshape(R, Cip, KK, Cop)[:, :Ci, :, :Co].transpose(0, 3, 1, 2).copy()
    return dwp.reshape(R, Cop, KK, Cip)[:, :Co, :, :Ci].transpose(0, 1, 3, 2).copy()


def flush(grad0, W, parts, u, v, sigma, dt=np.float64):
    """grad0 + (dW - <dW, W/sigma> u v^T)/sigma with dW = sum_r parts[r]; u None: grad0 + dW.  Returns (grad, inner)."""
    dW = _sum(parts.astype(dt), dt, axis=0).astype(dt)
    if u is None:
        return (grad0.astype(dt) + dW).astype(dt), dt(0.0)
    Co, Ci, KK = W.shape
    sigma = dt(sigma)
    inner = dt(dt(_sum((dW * W.astype(dt)).astype(dt), dt)) / sigma)
    uv = (u.astype(dt)[:, None] * v.astype(dt)[None, :]).astype(dt).reshape(Co, Ci, KK)
    g = ((dW - (inner * uv).astype(dt)).astype(dt) / sigma).astype(dt)
    return (grad0.astype(dt) + g).astype(dt), inner


def chain(W, u, v, grad0, parts, Cop, Cip, dt=np.float64):
    """Every quantity the weight bank computes for one weight, in the arithmetic dt:
    training prepare (u, v, sigma, wf, wb), eval prepare (sigma_eval, wf_eval, wb_eval), the flush after a training prepare
    (grad, inner; absent without staging)."""
    out = {}
    out["u"], out["v"], out["sigma"] = spectral(W, u, v, 1, dt)
    out["wf"], out["wb"] = pack(W, out["sigma"], Cop, Cip, dt)
    _, _, out["sigma_eval"] = spectral(W, u, v, 0, dt)
    out["wf_eval"], out["wb_eval"] = pack(W, out["sigma_eval"], Cop, Cip, dt)
    if parts is not None:
        out["grad"], out["inner"] = flush(grad0, W, parts, out["u"], out["v"], out["sigma"], dt)
    return out


def unpack_chain(W, u, v, sigma, grad0, dW, dt=np.float64):
    """ast_weight_grad_unpack on its own: ONE staging copy dW and a given float32 state (u, v, sigma) -- with spectral norm
    ("unpack") and as the plain unpack-accumulate of a weight without u ("unpack_plain")."""
    return {"unpack": flush(grad0, W, dW[None], u, v, sigma, dt)[0], "unpack_plain": flush(grad0, W, dW[None], None, None, 1.0, dt)[0]}


# ---- tolerances --------------------------------------------------------------------------------------------------------

QUANTITIES = ("u", "v", "sigma", "wf", "sigma_eval", "wf_eval", "grad", "unpack", "unpack_plain")


def e_seq(ref64, seq32):
    """per quantity: max |sequential-float32 chain - float64| / max |float64|"""
    out = {}
    for q in QUANTITIES:
        if q in ref64 and ref64[q] is not None:
            r = np.asarray(ref64[q], np.float64)
            out[q] = float(np.max(np.abs(np.asarray(seq32[q], np.float64) - r)) / np.max(np.abs(r)))
    return out


def bound_rel(e):
    """The f32 bound as a fraction of the float64 tensor's max-abs: min(2e-4, max(4 e_seq, 16 * 2^-24)).
    The device's add chains (at most ~72 elements per lane, then a tree) are shorter than the sequential chain e_seq is measured
    on; 4 covers a different realisation of the roundings; 16 * 2^-24 is the floor for quantities that are a handful of
    operations deep, where e_seq of one seeded draw can come out at an ulp or at zero."""
    return min(F32_CEILING, max(4.0 * e, 16.0 * U24))


def check(got, ref, rel, bf16=False):
    """(ok, worst |got - ref| / max|ref|, number outside): |got - ref| <= rel * max|ref| (+ 2^-8 |ref| for a bf16 value: one
    bf16 ulp, for an f32 value that lands across a rounding tie).  NaN in got counts as outside."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    scale = float(np.max(np.abs(ref)))
    err = np.abs(got - ref)
    lim = rel * scale + (BF16_ULP * np.abs(ref) if bf16 else 0.0)
    bad = ~(err <= lim)
    worst = float(np.max(np.where(np.isnan(err), np.inf, err))) / scale
    return not bool(bad.any()), worst, int(bad.sum())
