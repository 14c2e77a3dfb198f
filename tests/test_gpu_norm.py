"""The normalisation kernels of csrc/norm.hip against the float64 references of tests/norm_ref.py, through the C ABI and through
ops: channel statistics, finalize, apply and backward passes of BatchNorm2d / InstanceNorm2d, their fused-finalize twins
(ast_bn_apply_fwd / _bwd), the deterministic forms, LayerNorm and the fused residual + dropout + LayerNorm.  The case tables, seeded
inputs and bounds are norm_ref's; tests/test_norm_cpu.py checks the references, the conditions on the inputs and the launch
arithmetic below without a GPU.  The _len kernels keep their own suite (test_gpu_ragged_bn.py).

Which path the named cases enter (norm_ref.PATH_CLAIMS, asserted in test_norm_cpu.py):
  c24, c24-r8   U = 3: 256 % U != 0, so affine_act / norm_bwd_apply / bn_apply_* reload coef(j % U) every iteration; the reduction
                runs 85 pixel lanes and leaves one thread idle; 2 workgroups per image of 59 and 58 pixels (a ragged last block)
  c40-r2        U = 5, the same paths with 51 lanes and 32 workgroups per image
  c8-pad        U = 1, PL = 256 > HW = 117: lanes without a pixel; channels 2..7 are padding
  c2048         U = 256, PL = 1;  c256: nparts = 1, PL = 8 > HW = 3
  many-images   N = 600 > reduce_blocks(): one workgroup per image, the finalize lanes loop over the images
  stride2       N = 256, HW = 300, C = 64: elem_blocks() / N = 8 workgroups of 256 threads per image for 2400 units: a second trip
  hw3-det       HW = 3 < 64 slots: 61 slots per image hold no pixel and must still store zeros
  slot tables   rows x C = 1 x 64, 8 x 24, 16 x 24, 64 x 8, 32 x 2048 (the largest accepted): nparts = 1, 8, 10, 32, 1

Every kernel is chained the way ops chains it: the statistics table that ast_chan_stats wrote feeds ast_norm_finalize, its
coefficients feed ast_affine_act, and so on, and every output is compared with the one float64 reference of the case.  The bound of
a comparison is norm_ref.bound: max(8 * e32, 64 * 2^-24 * max(1, kappa / 4)) relative to max |reference|, 2^-8 more for a bf16
tensor a kernel stores; what is exact by construction (repeated deterministic calls, sentinel bands, padded channels, a table handed
back zero or left untouched, num_batches_tracked) is compared with torch.equal.  Every comparison prints err / e32 / bound; the
worst per group as measured on the MI355X (kernel error / e32 of that comparison / its bound):

                  all cases (the worst is a bf16 store)   float32 cases only
  chan_stats      3.17e-07 / 4.81e-08 / 3.81e-06          the same (c8-pad sums1)
  det_sums        3.26e-07 / 4.48e-08 / 3.81e-06          1.84e-07 / 4.50e-08 / 3.81e-06
  finalize        1.09e-06 / 1.51e-07 / 5.28e-06          the same (c40-r2 shift1)
  affine_act      3.37e-03 / 1.61e-07 / 3.91e-03          1.12e-06 / 1.39e-07 / 3.81e-06   (c512-const, linear)
  bwd_sums        2.51e-07 / 7.26e-08 / 3.81e-06          the same (c8-pad)
  bwd_finalize    2.33e-06 / 3.01e-07 / 5.28e-06          2.06e-06 / 7.68e-07 / 6.15e-06   (c40-r2 k1[2])
  bwd_apply       3.22e-03 / 9.34e-08 / 3.91e-03          1.40e-04 / 1.60e-07 / 1.27e-03   (c64-r32 dx)
  bn_apply        3.37e-03 / 1.61e-07 / 3.91e-03          1.14e-06 / 1.37e-07 / 5.28e-06   (c40-r2 shift1)
  autograd        3.22e-03 / 9.34e-08 / 3.91e-03          7.64e-06 / 1.36e-07 / 7.53e-05   (c24-r8 bn_act dx)
  layernorm       8.00e-07 / 8.00e-07 / 6.40e-06
  add_drop_ln     2.30e-06 / 1.23e-07 / 3.81e-06          (the mean of one 64-wide row: a sum that nearly cancels)

The raw-moment variance E[x^2] - m^2, measured in float32, the worse of the two variants of each case (error of rstd / y / dx, and
their bound): mean / std = 2: 4.9e-07 / 8.4e-07 / 5.3e-07, 5.3e-06; mean / std = 8: 8.2e-06 / 7.3e-06 / 7.6e-06, 7.5e-05; mean / std = 32:
9.0e-05 / 1.1e-04 / 1.4e-04, 1.3e-03.  The sums are added with atomics, so these figures move from run to run (rstd at 32: 7.9e-05 ...
1.6e-04 in three runs).  Torch's Welford stays at 3e-08 ... 1.2e-06 on the same inputs.  The error grows with kappa as the bound
assumes and uses about a tenth of it.

No kernel missed its bound, and csrc/norm.hip is unchanged.  One rule of this file was wrong on its first run and was corrected:
LayerNorm's dx at D = 1 is exactly 0 in the formula because rstd (g - mean(g) - xh mean(g xh)) cancels term by term, and the
reference being all zero the comparison asked for an exact 0.  ast_layernorm_bwd gives one; ast_add_drop_ln_bwd, where the compiler
contracts dy * gamma - mean(g) into one fma, leaves 4e-08 of the cancelling terms (rstd = eps^-1/2 = 316 times |dy gamma|).  That is
rounding at the scale of the terms, so a reference that is zero by cancellation is now held to the floor of the bound, 64 * 2^-24,
relative to the size of those terms (_close, `terms`); every other all-zero reference must still be met exactly.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

import norm_ref as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ast_amd import _lib, config, layers as AL, ops

DEV = "cuda"
GUARD = 64
SENTINEL = -24576.0           # representable in bf16
NAN = float("nan")
F64 = torch.float64
F32 = torch.float32
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nworst comparison per group: kernel error / float32 floor e32 / bound")
    for g, (err, e32, tol) in sorted(WORST.items()):
        print(f"  {g:<22} {err:.2e} / {e32:.2e} / {tol:.2e}")
    _case.cache_clear()


def _close(group, what, got, ref, plain32, kappa=1.0, bf16_store=False, terms=None):
    """[] or one line of failure: got within the measured bound of the float64 ref.  A ref that is all zero must be met exactly,
    unless it is zero because terms of size `terms` cancel (LayerNorm's dx at D = 1: rstd (g - mean(g) - xh mean(g xh)) with
    xh = 0 and mean(g) = g): then the floor of the bound, 64 * 2^-24, holds relative to `terms`, the scale the rounding happens at."""
    got, ref = torch.as_tensor(got).detach().cpu(), torch.as_tensor(ref).detach().cpu()
    assert got.numel() == ref.numel(), (what, tuple(got.shape), tuple(ref.shape))
    if not bool(torch.isfinite(got.float()).all()):
        return [f"{what}: {int((~torch.isfinite(got.float())).sum())} of {got.numel()} values are not finite"]
    if R.is_zero(ref) and terms is not None:
        err = float(got.double().abs().max()) / terms
        print(f"{group:<14} {what:<60} err {err:.2e} of the cancelling terms ({terms:.3g}), bound {R.FLOOR:.2e}")
        return [] if err <= R.FLOOR else [f"{what}: the reference is exactly 0 by cancellation of terms of {terms:.3g}, the kernel is {err:.3g} of that off"]
    if R.is_zero(ref):
        return [] if float(got.float().abs().max()) == 0.0 else [f"{what}: the reference is exactly 0, the kernel gives up to {float(got.float().abs().max()):.3g}"]
    e32, tol = R.bound(plain32, ref, kappa, bf16_store)
    err = R.rel(got, ref)
    print(f"{group:<14} {what:<60} err {err:.2e}   e32 {e32:.2e}   bound {tol:.2e}")
    if group not in WORST or err / tol > WORST[group][0] / WORST[group][2]:
        WORST[group] = (err, e32, tol)
    return [] if err <= tol else [f"{what}: {err:.3g} of max|ref| from the float64 reference, bound {tol:.3g} (float32 evaluation: {e32:.3g})"]


class _Buf:
    """n elements of `dtype` between two sentinel bands, in one allocation; off: elements by which the payload is shifted"""

    def __init__(self, n, dtype=None, fill=NAN, off=0):
        dtype = dtype or F32
        self.all = torch.full((n + off + 2 * GUARD,), int(SENTINEL) if dtype == torch.int64 else SENTINEL, dtype=dtype, device=DEV)
        self.t = self.all[GUARD + off:GUARD + off + n]
        self.t.fill_(fill)
        self.lo, self.hi = GUARD + off, GUARD

    def guards_intact(self):
        return bool((self.all[:self.lo] == SENTINEL).all()) and bool((self.all[-self.hi:] == SENTINEL).all())

    def from_(self, src):
        self.t.copy_(src.reshape(-1).to(self.t.dtype))
        return self


def _intact(*bufs):
    return all(b.guards_intact() for b in bufs if b is not None)


def _p(b):
    """device pointer of a _Buf, a tensor or None"""
    return None if b is None else _lib.ptr(b.t if isinstance(b, _Buf) else b)


def _call(name, *args):
    _lib.check(getattr(_lib.lib(), name)(*args, _lib.stream()), name)


def _prior(n, lo=-1.5, hi=2.5):
    """distinct non-zero float32 starting values of something a kernel ADDS onto"""
    return torch.linspace(lo, hi, n, dtype=F32) + 0.125


# ---- one BatchNorm / InstanceNorm case on the device ---------------------------------------------------------------------------

class _Case:
    def __init__(self, name, dtype, relu, with_r):
        self.name, self.dtype, self.relu = name, dtype, relu
        self.i = i = R.bn_inputs(name, dtype, relu, with_r)                                # this variant's own, separately conditioned inputs
        self.with_r = i["r"] is not None
        self.ref, self.plain, self.kappa = R.bn_reference(name, dtype, relu, self.with_r)
        self.N, self.HW, self.C, self.Creal = i["N"], i["HW"], i["C"], i["Creal"]
        self.n, self.cnt = self.N * self.HW * self.C, self.N * self.HW
        self.dt, self.bf16 = _lib.dcode(dtype), dtype == torch.bfloat16
        self.x, self.dy = (i[k].to(dtype).to(DEV).contiguous() for k in ("x", "dy"))
        self.r = i["r"].to(dtype).to(DEV).contiguous() if self.with_r else None
        self.p = {k: i[k].float().to(DEV) for k in ("g1", "b1", "g2", "b2", "rm", "rv")}
        self.tag = f"{name} {'bf16' if self.bf16 else 'f32'}{'' if relu else ' linear'}{' +IN' if self.with_r else ''}"

    def cmp(self, group, what, got, key, sel=None, prior=None):
        """got against the reference quantity `key` (sel: a function picking the same part of reference and float32 evaluation;
        prior: float32 values the kernel added onto)"""
        ref, plain = self.ref[key], self.plain[key]
        if sel is not None:
            ref, plain = sel(ref), sel(plain)
        if prior is not None:
            ref, plain = prior.double().reshape(ref.shape) + ref, prior.reshape(plain.shape) + plain
        return _close(group, f"{self.tag} {what}", torch.as_tensor(got).reshape(-1), ref.reshape(-1), plain.reshape(-1),
                      R.kappa_for(key, self.ref), self.bf16 and key in R.STORED_KEYS)

    def cmp_k(self, group, what, got, key):
        bad = []
        for q in range(3):                                  # the three coefficients differ by orders of magnitude
            bad += self.cmp(group, f"{what}[{q}]", got.reshape(-1, 3)[:, q], key, sel=lambda t: t[..., q])
        return bad

    # the chain ops runs, one stage each; every stage returns fresh sentinel-banded buffers
    def stats(self, src):
        tab = _Buf(self.N * self.C * 2)
        _call("ast_chan_stats", _p(src), _p(tab), self.N, self.HW, self.C, self.dt, 0)
        return tab

    def finalize(self, tab, instance, zero_sums=0, rm=None, rv=None, nbt=None, rows=None, HW=None, count=0, eval_mode=0):
        n = self.N * self.C if instance else self.C
        out = [_Buf(n) for _ in range(4)]
        k = "2" if instance else "1"
        _call("ast_norm_finalize", _p(tab), zero_sums, _p(nbt), self.N if rows is None else rows, self.HW if HW is None else HW, self.C, self.Creal,
              int(instance), _p(self.p["g" + k]), _p(self.p["b" + k]), _p(rm), _p(rv), eval_mode, R.EPS, *(_p(b) for b in out), count)
        return out

    def coefs(self):
        """(mean, rstd, scale, shift) of the batch branch and of the instance branch (or None), from the kernels"""
        c1 = self.finalize(self.stats(self.x), False)
        c2 = self.finalize(self.stats(self.r), True) if self.with_r else None
        return c1, c2

    def forward(self, c1, c2):
        y = _Buf(self.n, self.dtype)
        _call("ast_affine_act", _p(self.x), _p(c1[2]), _p(c1[3]), _p(self.r), _p(c2[2]) if c2 else None, _p(c2[3]) if c2 else None, _p(y),
              self.N, self.HW, self.C, int(self.relu), self.dt)
        return y

    def sums3(self, c1, c2, y=None, assume_zeroed=0, tab=None):
        """ast_norm_bwd_sums (mask from y) or ast_norm_bwd_sums_pre (mask from the pre-activation)"""
        tab = tab or _Buf(self.N * self.C * 3)
        if y is not None:
            _call("ast_norm_bwd_sums", _p(self.dy), _p(y), _p(self.x), _p(self.r), _p(tab), self.N, self.HW, self.C, int(self.relu), self.dt, assume_zeroed)
        else:
            _call("ast_norm_bwd_sums_pre", _p(self.dy), None, _p(self.x), _p(self.r), _p(tab), self.N, self.HW, self.C, int(self.relu), self.dt,
                  assume_zeroed, _p(c1[2]), _p(c1[3]), _p(c2[2]) if c2 else None, _p(c2[3]) if c2 else None)
        return tab

    def check_padding(self, what, t, last=None):
        """channels >= Creal of an activation-shaped (or [.., C, last]) output are exact zeros"""
        if self.Creal == self.C:
            return []
        v = t.reshape(-1, self.C, last)[:, self.Creal:] if last else t.reshape(-1, self.C)[:, self.Creal:]
        return [] if float(v.float().abs().max()) == 0.0 else [f"{self.tag} {what}: padded channels are not zero"]


@functools.lru_cache(maxsize=None)
def _case(name, dtype, relu=True, with_r=True):
    return _Case(name, dtype, relu, with_r)


BN = pytest.mark.parametrize("name,dtype", R.BN_PARAMS, ids=R.BN_IDS)


# ---- 1. ast_chan_stats / ast_chan_stats_det ------------------------------------------------------------------------------------

@BN
def test_chan_stats(name, dtype):
    g = _case(name, dtype)
    bad = []
    for src, key in ((g.x, "sums1"),) + (((g.r, "sums2"),) if g.with_r else ()):
        tab = g.stats(src)                                   # assume_zeroed = 0 clears the NaN fill first
        bad += g.cmp("chan_stats", f"ast_chan_stats {key}", tab.t, key)
        prior = _prior(g.N * g.C * 2)
        tab2 = _Buf(g.N * g.C * 2).from_(prior)
        _call("ast_chan_stats", _p(src), _p(tab2), g.N, g.HW, g.C, g.dt, 1)          # assume_zeroed = 1 adds onto what is there
        bad += g.cmp("chan_stats", f"ast_chan_stats {key} onto a filled table", tab2.t, key, prior=prior)
        assert _intact(tab, tab2)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("dtype", R.BOTH, ids=["f32", "bf16"])
@pytest.mark.parametrize("name", R.DET_CASES)
def test_deterministic_sums(name, dtype):
    """ast_chan_stats_det / ast_norm_bwd_sums_det at 1, 3 and 64 slots: two calls give the same bits; with at most one pixel per lane
    (HW <= PL) every slot count adds the same terms in the same order, so the results are equal across slot counts too; slots
    beyond the last pixel store zeros."""
    g = _case(name, dtype)
    c1, c2 = g.coefs()
    one_pixel_per_lane = g.HW <= R.reduce_launch(g.N, g.HW, g.C)["PL"] and all(
        R.reduce_launch(g.N, g.HW, g.C, s)["ppb"] == 1 or s == 1 for s in R.DET_SLOTS)
    bad, results = [], {}
    for slots in R.DET_SLOTS:
        empty = R.reduce_launch(g.N, g.HW, g.C, slots)["empty_slots"]
        for K, key in ((2, "sums1"), (3, "sums3")):
            runs = []
            for _ in range(2):
                ws, out = _Buf(g.N * slots * g.C * K), _Buf(g.N * g.C * K)
                if K == 2:
                    _call("ast_chan_stats_det", _p(g.x), _p(out), g.N, g.HW, g.C, g.dt, _p(ws), slots)
                else:
                    _call("ast_norm_bwd_sums_det", _p(g.dy), None, _p(g.x), _p(g.r), _p(out), g.N, g.HW, g.C, 1, g.dt, _p(c1[2]), _p(c1[3]),
                          _p(c2[2]) if c2 else None, _p(c2[3]) if c2 else None, _p(ws), slots)
                assert _intact(ws, out)
                runs.append(out.t.cpu())
                if empty:
                    tail = ws.t.view(g.N, slots, g.C * K)[:, slots - empty:]
                    if not torch.equal(tail.cpu(), torch.zeros(g.N, empty, g.C * K)):
                        bad.append(f"{g.tag} {key} slots={slots}: a slot without a pixel does not hold zeros")
            if not torch.equal(runs[0], runs[1]):
                bad.append(f"{g.tag} {key} slots={slots}: two runs differ")
            bad += g.cmp("det_sums", f"{key} det slots={slots}", runs[0], key)
            results[(key, slots)] = runs[0]
    if one_pixel_per_lane:
        for key in ("sums1", "sums3"):
            for slots in R.DET_SLOTS[1:]:
                if not torch.equal(results[(key, slots)], results[(key, R.DET_SLOTS[0])]):
                    bad.append(f"{g.tag} {key}: {slots} slots and {R.DET_SLOTS[0]} add the same terms in the same order but differ")
    assert not bad, "\n".join(bad)


# ---- 2. ast_norm_finalize ------------------------------------------------------------------------------------------------------

@BN
def test_norm_finalize(name, dtype):
    g = _case(name, dtype)
    bad = []
    tab = g.stats(g.x)
    before = tab.t.clone()
    rm, rv, nbt = _Buf(g.Creal).from_(g.p["rm"]), _Buf(g.Creal).from_(g.p["rv"]), _Buf(1, torch.int64, 0)
    out = g.finalize(tab, False, 0, rm, rv, nbt)
    assert torch.equal(tab.t, before), "zero_sums = 0 must leave the table untouched"
    assert int(nbt.t) == 1
    for b, key in zip(out, ("mean1", "rstd1", "scale1", "shift1")):
        bad += g.cmp("finalize", f"ast_norm_finalize {key}", b.t, key)
    bad += g.cmp("finalize", "running_mean", rm.t, "running_mean") + g.cmp("finalize", "running_var", rv.t, "running_var")
    bad += g.check_padding("scale", out[2].t) + g.check_padding("shift", out[3].t)
    assert _intact(tab, rm, rv, nbt, *out)
    # running statistics and the counter are optional; zero_sums = 1 hands the table back exactly zero
    out2 = g.finalize(tab, False, 1, None, None, None)
    assert torch.equal(tab.t, torch.zeros_like(tab.t)) and _intact(tab, *out2)
    assert all(torch.equal(a.t, b.t) for a, b in zip(out, out2))
    if g.i["const"] is not None:
        c = g.i["const"]
        assert float(out[0].t[c]) == 0.5 and abs(float(out[1].t[c]) - R.EPS ** -0.5) <= R.FLOOR * R.EPS ** -0.5
    if g.with_r:                                             # InstanceNorm2d: one statistic per (image, channel)
        tab = g.stats(g.r)
        before = tab.t.clone()
        out = g.finalize(tab, True, 0)
        assert torch.equal(tab.t, before)
        for b, key in zip(out, ("mean2", "rstd2", "scale2", "shift2")):
            bad += g.cmp("finalize", f"ast_norm_finalize instance {key}", b.t, key)
        bad += g.check_padding("scale2", out[2].t) + g.check_padding("shift2", out[3].t)
        out2 = g.finalize(tab, True, 1)
        assert torch.equal(tab.t, torch.zeros_like(tab.t)) and all(torch.equal(a.t, b.t) for a, b in zip(out, out2)) and _intact(tab, *out, *out2)
    # eval mode: the running statistics are the statistics; no table
    rm, rv = _Buf(g.Creal).from_(g.p["rm"]), _Buf(g.Creal).from_(g.p["rv"])
    out = g.finalize(None, False, 0, rm, rv, None, eval_mode=1)
    G1, B1 = (R.pad_params(g.i[k], g.C) for k in ("g1", "b1"))
    m64, v64 = R.pad_params(g.i["rm"], g.C), R.pad_params(g.i["rv"], g.C)
    v64[g.Creal:] = 1.0
    ref = (m64,) + R.finalize(m64, v64, G1, B1, R.EPS)
    p32 = (m64.float(),) + R.finalize(m64.float(), v64.float(), G1.float(), B1.float(), R.EPS)
    for b, r64, r32, key in zip(out, ref, p32, ("mean", "rstd", "scale", "shift")):
        bad += _close("finalize", f"{g.tag} eval {key}", b.t, r64, r32)
    assert torch.equal(rm.t.cpu(), g.i["rm"].float()) and torch.equal(rv.t.cpu(), g.i["rv"].float()) and _intact(rm, rv, *out)
    assert not bad, "\n".join(bad)


def _slot_tables(g, rows):
    """[rows][C][2] and [rows][C][3] float32 slot tables written from the float64 sums of the pixels dealt into the rows"""
    dz = g.ref["relu_bwd"]
    t2 = torch.stack([torch.stack([p.sum(0), (p * p).sum(0)], -1) for p in R.slot_split(g.i["x"], rows)])
    t3 = torch.stack([torch.stack([d.sum(0), (d * p).sum(0), torch.zeros(g.C, dtype=F64)], -1)
                      for d, p in zip(R.slot_split(dz, rows), R.slot_split(g.i["x"], rows))])
    return _Buf(rows * g.C * 2).from_(t2.float()), _Buf(rows * g.C * 3).from_(t3.float())


SLOTS = pytest.mark.parametrize("rows,name", R.SLOT_CASES, ids=[f"{r}x{n}" for r, n in R.SLOT_CASES])


@SLOTS
def test_finalize_from_slot_tables(rows, name):
    """count > 0: the table rows are partial-sum slots, the pixel count comes separately (HW is passed as 0)"""
    g = _case(name, torch.float32, True, False)
    tab2, tab3 = _slot_tables(g, rows)
    rm, rv, nbt = _Buf(g.Creal).from_(g.p["rm"]), _Buf(g.Creal).from_(g.p["rv"]), _Buf(1, torch.int64, 0)
    out = g.finalize(tab2, False, 1, rm, rv, nbt, rows=rows, HW=0, count=g.cnt)
    bad = []
    for b, key in zip(out, ("mean1", "rstd1", "scale1", "shift1")):
        bad += g.cmp("finalize", f"ast_norm_finalize {rows} slots {key}", b.t, key)
    bad += g.cmp("finalize", f"{rows} slots running_var", rv.t, "running_var")
    assert int(nbt.t) == 1 and torch.equal(tab2.t, torch.zeros_like(tab2.t)) and _intact(tab2, rm, rv, nbt, *out)
    k1, dg, db = _Buf(g.C * 3), _Buf(g.Creal).from_(_prior(g.Creal)), _Buf(g.Creal).from_(_prior(g.Creal, 0.5, 1.5))
    _call("ast_norm_bwd_finalize_n", _p(tab3), 1, rows, 0, g.C, g.Creal, _p(g.p["g1"]), _p(out[0]), _p(out[1]), _p(dg), _p(db), _p(k1),
          None, None, None, None, None, None, g.cnt)
    bad += g.cmp_k("bwd_finalize", f"ast_norm_bwd_finalize_n {rows} slots k1", k1.t, "k1")
    bad += g.cmp("bwd_finalize", f"{rows} slots dgamma", dg.t, "dgamma1", prior=_prior(g.Creal))
    bad += g.cmp("bwd_finalize", f"{rows} slots dbeta", db.t, "dbeta1", prior=_prior(g.Creal, 0.5, 1.5))
    assert torch.equal(tab3.t, torch.zeros_like(tab3.t)) and _intact(tab3, k1, dg, db)
    assert not bad, "\n".join(bad)


# ---- 3. ast_affine_act ---------------------------------------------------------------------------------------------------------

# the large case runs in one form only (norm_ref.ONE_VARIANT): no linear variant of it
AFFINE = [(n, d, relu) for n, d in R.BN_PARAMS for relu in (True, False) if relu or n not in R.ONE_VARIANT]


@pytest.mark.parametrize("name,dtype,relu", AFFINE,
                         ids=[f"{n}-{'f32' if d == torch.float32 else 'bf16'}-{'relu' if relu else 'linear'}" for n, d, relu in AFFINE])
def test_affine_act(name, dtype, relu):
    bad = []
    for with_r in R.variants(name):
        g = _case(name, dtype, relu, with_r)
        c1, c2 = g.coefs()
        y = g.forward(c1, c2)
        bad += g.cmp("affine_act", "ast_affine_act y", y.t, "y") + g.check_padding("y", y.t)
        assert _intact(y, *c1, *(c2 or ()))
        if g.with_r:                                        # relu bit 2: the FIRST input's scale is per image, [N][C]: relu?(IN(r))
            y2 = _Buf(g.n, dtype)
            _call("ast_affine_act", _p(g.r), _p(c2[2]), _p(c2[3]), None, None, None, _p(y2), g.N, g.HW, g.C, int(relu) | 2, g.dt)
            ref = g.i["r"] * g.ref["scale2"][:, None] + g.ref["shift2"][:, None]
            p32 = g.i["r"].float() * g.plain["scale2"][:, None] + g.plain["shift2"][:, None]
            if relu:
                ref, p32 = ref.clamp(min=0), p32.clamp(min=0)
            bad += _close("affine_act", f"{g.tag} per-image scale", y2.t, ref, p32, g.ref["kappa2"], g.bf16)
            assert _intact(y2)
    assert not bad, "\n".join(bad)


# ---- 4. backward: sums, finalize, apply ----------------------------------------------------------------------------------------

@BN
def test_norm_backward(name, dtype):
    bad = []
    for with_r in R.variants(name):
        g = _case(name, dtype, True, with_r)
        c1, c2 = g.coefs()
        y = g.forward(c1, c2)
        # the mask from y and the mask from the pre-activation give the same sums (no pre-activation is near zero)
        from_y = g.sums3(c1, c2, y=y)
        from_pre = g.sums3(c1, c2, assume_zeroed=1, tab=_Buf(g.N * g.C * 3, fill=0.0))
        for tab, how in ((from_y, "mask from y"), (from_pre, "mask from pre")):
            bad += g.cmp("bwd_sums", f"ast_norm_bwd_sums {how}", tab.t, "sums3")
        assert _intact(from_y, from_pre)
        before = from_pre.t.clone()
        # k1, k2 and the parameter gradients, added onto what is there; zero_sums = 0 leaves the table, 1 clears it
        pri = [_prior(g.Creal, a, b) for a, b in ((-1.5, 2.5), (0.5, 1.5), (-2.0, -1.0), (1.0, 3.0))]
        k1, k2 = _Buf(g.C * 3), _Buf(g.N * g.C * 3) if g.with_r else None
        grads = [_Buf(g.Creal).from_(p) for p in pri]
        _call("ast_norm_bwd_finalize", _p(from_pre), 0, g.N, g.HW, g.C, g.Creal, _p(g.p["g1"]), _p(c1[0]), _p(c1[1]), _p(grads[0]), _p(grads[1]), _p(k1),
              *((_p(g.p["g2"]), _p(c2[0]), _p(c2[1]), _p(grads[2]), _p(grads[3]), _p(k2)) if g.with_r else (None,) * 6))
        assert torch.equal(from_pre.t, before)
        bad += g.cmp_k("bwd_finalize", "k1", k1.t, "k1") + g.check_padding("k1", k1.t, 3)
        bad += g.cmp("bwd_finalize", "dgamma1 +=", grads[0].t, "dgamma1", prior=pri[0]) + g.cmp("bwd_finalize", "dbeta1 +=", grads[1].t, "dbeta1", prior=pri[1])
        if g.with_r:
            bad += g.cmp_k("bwd_finalize", "k2", k2.t, "k2") + g.check_padding("k2", k2.t, 3)
            bad += g.cmp("bwd_finalize", "dgamma2 +=", grads[2].t, "dgamma2", prior=pri[2]) + g.cmp("bwd_finalize", "dbeta2 +=", grads[3].t, "dbeta2", prior=pri[3])
        else:
            assert all(torch.equal(b.t.cpu(), p) for b, p in zip(grads[2:], pri[2:]))
        assert _intact(from_pre, k1, k2, *grads)
        k1b = _Buf(g.C * 3)
        _call("ast_norm_bwd_finalize", _p(from_y), 1, g.N, g.HW, g.C, g.Creal, _p(g.p["g1"]), _p(c1[0]), _p(c1[1]), None, None, _p(k1b),
              *(None,) * 6)
        assert torch.equal(from_y.t, torch.zeros_like(from_y.t)) and _intact(from_y, k1b)
        bad += g.cmp_k("bwd_finalize", "k1 (no gradients, table cleared)", k1b.t, "k1")
        # apply: plain ReLU backward (k1 = NULL), dx, dx + dr; mask from y and from the pre-activation
        dz = _Buf(g.n, dtype)
        _call("ast_norm_bwd_apply", _p(g.dy), _p(y), None, None, None, None, _p(dz), None, g.N, g.HW, g.C, 1, g.dt)
        bad += g.cmp("bwd_apply", "ast_norm_bwd_apply k1 = NULL", dz.t, "relu_bwd")
        for how in ("y", "pre"):
            dx, dr = _Buf(g.n, dtype), _Buf(g.n, dtype) if g.with_r else None
            if how == "y":
                _call("ast_norm_bwd_apply", _p(g.dy), _p(y), _p(g.x), _p(g.r), _p(k1), _p(k2), _p(dx), _p(dr), g.N, g.HW, g.C, 1, g.dt)
            else:
                _call("ast_norm_bwd_apply_pre", _p(g.dy), None, _p(g.x), _p(g.r), _p(k1), _p(k2), _p(dx), _p(dr), g.N, g.HW, g.C, 1, g.dt,
                      _p(c1[2]), _p(c1[3]), _p(c2[2]) if c2 else None, _p(c2[3]) if c2 else None)
            bad += g.cmp("bwd_apply", f"dx (mask from {how})", dx.t, "dx") + g.check_padding("dx", dx.t)
            if g.with_r:
                bad += g.cmp("bwd_apply", f"dr (mask from {how})", dr.t, "dr") + g.check_padding("dr", dr.t)
            assert _intact(dx, dr, dz)
        if g.with_r:                                        # dx alone while the second input still shapes the mask
            dx = _Buf(g.n, dtype)
            _call("ast_norm_bwd_apply_pre", _p(g.dy), None, _p(g.x), _p(g.r), _p(k1), None, _p(dx), None, g.N, g.HW, g.C, 1, g.dt,
                  _p(c1[2]), _p(c1[3]), _p(c2[2]), _p(c2[3]))
            bad += g.cmp("bwd_apply", "dx only, two inputs", dx.t, "dx")
            assert _intact(dx)
    assert not bad, "\n".join(bad)


# ---- 5. ast_bn_apply_fwd / ast_bn_apply_bwd ------------------------------------------------------------------------------------

def _bn_apply_fwd(g, tab1, rows, tab2, rm, rv, nbt, relu=1):
    y, out1, out2 = _Buf(g.n, g.dtype), _Buf(4 * g.C), _Buf(4 * g.N * g.C) if g.with_r else None
    rc = _lib.lib().ast_bn_apply_fwd(_p(g.x), _p(g.r), _p(y), _p(tab1), rows, g.cnt, _p(tab2), _p(g.p["g1"]), _p(g.p["b1"]), _p(rm), _p(rv), _p(nbt),
                                     R.EPS, _p(g.p["g2"]) if g.with_r else None, _p(g.p["b2"]) if g.with_r else None, R.EPS, _p(out1), _p(out2),
                                     g.N, g.HW, g.C, g.Creal, relu, g.dt, _lib.stream())
    return rc, y, out1, out2


def _bn_apply_bwd(g, tab3, rows, out1, out2, grads, relu=1):
    dx, dr = _Buf(g.n, g.dtype), _Buf(g.n, g.dtype) if g.with_r else None
    o1 = out1.t.view(4, g.C)
    o2 = out2.t.view(4, g.N * g.C) if g.with_r else [None] * 4
    rc = _lib.lib().ast_bn_apply_bwd(_p(g.dy), _p(g.x), _p(g.r), _p(dx), _p(dr), _p(tab3), rows, g.cnt, _p(g.p["g1"]), _p(o1[0]), _p(o1[1]),
                                     _p(grads[0]), _p(grads[1]), _p(g.p["g2"]) if g.with_r else None, _p(o2[0]), _p(o2[1]), _p(grads[2]),
                                     _p(grads[3]), _p(o1[2]), _p(o1[3]), _p(o2[2]), _p(o2[3]), g.N, g.HW, g.C, g.Creal, relu, g.dt, _lib.stream())
    return rc, dx, dr


def _check_fused(g, group, what, rows, tab1, tab2, tab3):
    """one ast_bn_apply_fwd and one ast_bn_apply_bwd launch against the references of groups 2-4"""
    bad = []
    keep = [t.t.clone() for t in (tab1, tab2, tab3) if t is not None]
    rm, rv, nbt = _Buf(g.Creal).from_(g.p["rm"]), _Buf(g.Creal).from_(g.p["rv"]), _Buf(1, torch.int64, 0)
    rc, y, out1, out2 = _bn_apply_fwd(g, tab1, rows, tab2, rm, rv, nbt)
    _lib.check(rc, "ast_bn_apply_fwd")
    bad += g.cmp(group, f"{what} y", y.t, "y") + g.check_padding("y", y.t)
    for q, key in enumerate(("mean1", "rstd1", "scale1", "shift1")):
        bad += g.cmp(group, f"{what} out1 {key}", out1.t.view(4, g.C)[q], key)
        if g.with_r:
            bad += g.cmp(group, f"{what} out2 {key[:-1]}2", out2.t.view(4, -1)[q], key[:-1] + "2")
    # the lead workgroup alone moves the running statistics, by one momentum step, and the counter by one
    bad += g.cmp(group, f"{what} running_mean", rm.t, "running_mean") + g.cmp(group, f"{what} running_var", rv.t, "running_var")
    if int(nbt.t) != 1:
        bad.append(f"{g.tag} {what}: num_batches_tracked is {int(nbt.t)} after one call")
    pri = [_prior(g.Creal, a, b) for a, b in ((-1.5, 2.5), (0.5, 1.5), (-2.0, -1.0), (1.0, 3.0))]
    grads = [_Buf(g.Creal).from_(p) for p in pri]
    rc, dx, dr = _bn_apply_bwd(g, tab3, rows, out1, out2, grads if g.with_r else grads[:2] + [None, None])
    _lib.check(rc, "ast_bn_apply_bwd")
    bad += g.cmp(group, f"{what} dx", dx.t, "dx") + g.check_padding("dx", dx.t)
    bad += g.cmp(group, f"{what} dgamma1 +=", grads[0].t, "dgamma1", prior=pri[0]) + g.cmp(group, f"{what} dbeta1 +=", grads[1].t, "dbeta1", prior=pri[1])
    if g.with_r:
        bad += g.cmp(group, f"{what} dr", dr.t, "dr") + g.check_padding("dr", dr.t)
        bad += g.cmp(group, f"{what} dgamma2 +=", grads[2].t, "dgamma2", prior=pri[2]) + g.cmp(group, f"{what} dbeta2 +=", grads[3].t, "dbeta2", prior=pri[3])
    tabs = [t for t in (tab1, tab2, tab3) if t is not None]
    if not all(torch.equal(t.t, k) for t, k in zip(tabs, keep)):
        bad.append(f"{g.tag} {what}: a statistics table was written")
    assert _intact(y, out1, out2, rm, rv, nbt, dx, dr, *grads, *tabs)
    return bad


@BN
def test_bn_apply(name, dtype):
    """per-image tables (rows = N) from ast_chan_stats and ast_norm_bwd_sums_pre, with and without the InstanceNorm input"""
    bad = []
    for with_r in R.variants(name):
        g = _case(name, dtype, True, with_r)
        c1, c2 = g.coefs()
        grid = R.elem_launch(g.N, g.HW, g.C)["grid"]
        bad += _check_fused(g, "bn_apply", f"ast_bn_apply grid {grid[0]}x{grid[1]}", g.N, g.stats(g.x), g.stats(g.r) if g.with_r else None,
                            g.sums3(c1, c2))
    assert not bad, "\n".join(bad)


@SLOTS
def test_bn_apply_from_slot_tables(rows, name):
    g = _case(name, torch.float32, True, False)
    tab2, tab3 = _slot_tables(g, rows)
    a = R.apply_launch(rows, g.C)
    bad = _check_fused(g, "bn_apply", f"ast_bn_apply {rows} slots nparts {a['nparts']}", rows, tab2, None, tab3)
    assert not bad, "\n".join(bad)


def test_bn_apply_refuses_a_table_past_its_limit():
    """rows * C = 65536 + C: -1 from both entries, nothing launched, every output still at its fill value"""
    rows, name = R.SLOT_REJECTED
    g = _case(name, torch.float32, True, False)
    assert rows * g.C == 65536 + g.C
    tab2, tab3 = _Buf(rows * g.C * 2, fill=0.0), _Buf(rows * g.C * 3, fill=0.0)
    rm, rv, nbt = _Buf(g.Creal).from_(g.p["rm"]), _Buf(g.Creal).from_(g.p["rv"]), _Buf(1, torch.int64, 0)
    rc, y, out1, _ = _bn_apply_fwd(g, tab2, rows, None, rm, rv, nbt)
    assert rc == -1 and b"ast_bn_apply_fwd" in _lib.lib().ast_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(y.t).all()) and bool(torch.isnan(out1.t).all()) and int(nbt.t) == 0
    assert torch.equal(rm.t, g.p["rm"]) and torch.equal(rv.t, g.p["rv"])
    out1.t.fill_(1.0)
    grads = [_Buf(g.Creal).from_(_prior(g.Creal)) for _ in range(2)]
    rc, dx, _ = _bn_apply_bwd(g, tab3, rows, out1, None, grads + [None, None])
    assert rc == -1 and b"ast_bn_apply_bwd" in _lib.lib().ast_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(dx.t).all()) and all(torch.equal(b.t.cpu(), _prior(g.Creal)) for b in grads)


# ---- 6. through autograd -------------------------------------------------------------------------------------------------------

@pytest.fixture(params=[True, False], ids=["fused-finalize", "separate-finalize"])
def fused_finalize(request):
    old = config.fused_finalize
    config.fused_finalize = request.param
    yield request.param
    config.fused_finalize = old


def _modules(g):
    bn, inn = nn.BatchNorm2d(g.Creal, eps=R.EPS, momentum=R.MOMENTUM).to(DEV), nn.InstanceNorm2d(g.Creal, eps=R.EPS, affine=True).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(g.p["g1"]); bn.bias.copy_(g.p["b1"]); bn.running_mean.copy_(g.p["rm"]); bn.running_var.copy_(g.p["rv"])
        inn.weight.copy_(g.p["g2"]); inn.bias.copy_(g.p["b2"])
    return bn, inn


@pytest.mark.parametrize("dtype", R.BOTH, ids=["f32", "bf16"])
@pytest.mark.parametrize("name", R.AUTOGRAD_CASES)
def test_through_autograd(name, dtype, fused_finalize):
    """AL.bn_act and ops.ResTailFn, what the encoders run, at C = 24 and at mean / std = 8 against the same float64 references"""
    bad = []
    H, W = 9, 13
    for with_r in (False, True):
        g = _case(name, dtype, True, with_r)
        assert g.HW == H * W
        bn, inn = _modules(g)
        shape = (g.N, H, W, g.C)
        xh = g.x.view(shape).clone().requires_grad_(True)
        if with_r:
            rh = g.r.view(shape).clone().requires_grad_(True)
            y = ops.ResTailFn.apply(xh, rh, bn.weight, bn.bias, inn.weight, inn.bias, bn, inn, True)
            what = "ResTailFn"
        else:
            y = AL.bn_act(xh, bn, True, relu=True)
            what = "bn_act"
        y.backward(g.dy.view(shape))
        bad += g.cmp("autograd", f"{what} y", y, "y") + g.cmp("autograd", f"{what} dx", xh.grad, "dx")
        bad += g.cmp("autograd", f"{what} dgamma1", bn.weight.grad, "dgamma1") + g.cmp("autograd", f"{what} dbeta1", bn.bias.grad, "dbeta1")
        bad += g.cmp("autograd", f"{what} running_mean", bn.running_mean, "running_mean")
        bad += g.cmp("autograd", f"{what} running_var", bn.running_var, "running_var")
        assert int(bn.num_batches_tracked) == 1
        if with_r:
            bad += g.cmp("autograd", f"{what} dr", rh.grad, "dr")
            bad += g.cmp("autograd", f"{what} dgamma2", inn.weight.grad, "dgamma2") + g.cmp("autograd", f"{what} dbeta2", inn.bias.grad, "dbeta2")
    assert not bad, "\n".join(bad)


# ---- 7. LayerNorm ----------------------------------------------------------------------------------------------------------------

def _ln_plain32(i, mask=None, with_x=True, with_ln=True, with_dy=True, with_ds=True):
    """float32 torch: s = x + mask * sub, y = layer_norm(s), gradients of <y, dy> + <s, ds_ext> -> dict"""
    x, sub = i["x"].float().requires_grad_(True), i["sub"].float().requires_grad_(True)
    g, b = i["gamma"].float().requires_grad_(True), i["beta"].float().requires_grad_(True)
    s = sub * mask.float() if mask is not None else sub * 1.0
    if with_x:
        s = s + x
    o = {"s": s.detach()}
    loss = (s * i["ds_ext"].float()).sum() if with_ds else 0.0
    if with_ln:
        y, m, rs = torch.native_layer_norm(s, (s.shape[-1],), g, b, R.EPS)
        o.update(y=y.detach(), mean=m.detach().reshape(-1), rstd=rs.detach().reshape(-1))
        if with_dy:
            loss = loss + (y * i["dy"].float()).sum()
    gr = torch.autograd.grad(loss, [s, sub, g, b], allow_unused=True)                     # dx = ds, whether or not x took part
    o.update(dx=gr[0], dsub=gr[1], dgamma=gr[2], dbeta=gr[3])
    return o


@pytest.mark.parametrize("D", R.LN_D)
@pytest.mark.parametrize("rows", R.LN_ROWS)
def test_layernorm(rows, D):
    i = R.ln_inputs(rows, D)
    y64, m64, rs64 = R.layernorm(i["x"], i["gamma"], i["beta"])
    dx64, dg64, db64 = R.layernorm_bwd(i["dy"], i["x"], i["gamma"], m64, rs64)
    x32 = i["x"].float().requires_grad_(True)
    g32, b32 = i["gamma"].float().requires_grad_(True), i["beta"].float().requires_grad_(True)
    y32, m32, rs32 = torch.native_layer_norm(x32, (D,), g32, b32, R.EPS)
    dx32, dg32, db32 = torch.autograd.grad(y32, [x32, g32, b32], i["dy"].float())
    x, dy, gamma, beta = (i[k].float().to(DEV) for k in ("x", "dy", "gamma", "beta"))
    y, mean, rstd = _Buf(rows * D), _Buf(rows), _Buf(rows)
    _call("ast_layernorm_fwd", _p(x), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), rows, D, R.EPS, _lib.F32)
    what = f"rows={rows} D={D}"
    bad = _close("layernorm", f"{what} y", y.t, y64, y32.detach()) + _close("layernorm", f"{what} mean", mean.t, m64, m32.reshape(-1))
    bad += _close("layernorm", f"{what} rstd", rstd.t, rs64, rs32.reshape(-1))
    assert _intact(y, mean, rstd)
    pg, pb = i["dgamma0"].float(), i["dbeta0"].float()
    outs = []
    for det in (0, 1, 2):                                   # the atomic form, the deterministic form twice
        dx, dg, db, ws = _Buf(rows * D), _Buf(D).from_(pg), _Buf(D).from_(pb), _Buf(2 * rows * D)
        if det:
            _call("ast_layernorm_bwd_det", _p(dy), _p(x), _p(gamma), _p(mean), _p(rstd), _p(dx), _p(dg), _p(db), rows, D, _lib.F32, _p(ws))
        else:
            _call("ast_layernorm_bwd", _p(dy), _p(x), _p(gamma), _p(mean), _p(rstd), _p(dx), _p(dg), _p(db), rows, D, _lib.F32)
        form = "det" if det else "atomic"
        bad += _close("layernorm", f"{what} dx {form}", dx.t, dx64, dx32, terms=float(rs64.max() * (i["dy"] * i["gamma"]).abs().max()))
        bad += _close("layernorm", f"{what} dgamma += {form}", dg.t, i["dgamma0"] + dg64, pg + dg32)
        bad += _close("layernorm", f"{what} dbeta += {form}", db.t, i["dbeta0"] + db64, pb + db32)
        assert _intact(dx, dg, db, ws)
        outs.append((dx.t.cpu(), dg.t.cpu(), db.t.cpu()))
    assert all(torch.equal(a, b) for a, b in zip(outs[1], outs[2])), "two deterministic runs differ"
    # dx alone: the parameter gradients are optional
    dx = _Buf(rows * D)
    _call("ast_layernorm_bwd", _p(dy), _p(x), _p(gamma), _p(mean), _p(rstd), _p(dx), None, None, rows, D, _lib.F32)
    assert torch.equal(dx.t.cpu(), outs[0][0]) and _intact(dx)
    assert not bad, "\n".join(bad)


def test_layernorm_is_float32_only():
    rows, D = 4, 64
    x = torch.zeros(rows * D, dtype=torch.bfloat16, device=DEV)
    g = torch.ones(D, device=DEV)
    y, m, r = _Buf(rows * D), _Buf(rows), _Buf(rows)
    L = _lib.lib()
    assert L.ast_layernorm_fwd(_p(x), _p(g), _p(g), _p(y), _p(m), _p(r), rows, D, R.EPS, _lib.BF16, _lib.stream()) == -1
    assert L.ast_layernorm_bwd(_p(x), _p(x), _p(g), _p(m), _p(r), _p(y), None, None, rows, D, _lib.BF16, _lib.stream()) == -1
    assert L.ast_layernorm_bwd_det(_p(x), _p(x), _p(g), _p(m), _p(r), _p(y), None, None, rows, D, _lib.BF16, _p(y), _lib.stream()) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(y.t).all()) and bool(torch.isnan(m.t).all()) and _intact(y, m, r)


# ---- 8. fused residual + dropout + LayerNorm --------------------------------------------------------------------------------------

ADLN_SHAPES = [(D, False) for D in R.LN_D] + [(256, True)]   # (256, True): one operand 4 bytes off 16-byte alignment -> the generic kernels


@pytest.mark.parametrize("rows", R.ADLN_ROWS)
@pytest.mark.parametrize("D,misaligned", ADLN_SHAPES, ids=[f"D{d}{'-misaligned' if m else ''}" for d, m in ADLN_SHAPES])
def test_add_drop_ln(D, misaligned, rows):
    from test_gpu_ops import host_dropout_mask
    i = R.ln_inputs(rows, D)
    n = rows * D
    off = 1 if misaligned else 0
    dev = {k: i[k].float().to(DEV).contiguous() for k in ("x", "gamma", "beta", "dy", "ds_ext")}
    sub = _Buf(n, off=off).from_(i["sub"].float())           # the forward's shifted operand
    assert (sub.t.data_ptr() % 16 != 0) == misaligned and all(t.data_ptr() % 16 == 0 for t in dev.values())
    d_off = torch.tensor([R.ADLN_OFFSET], dtype=torch.int64, device=DEV)
    bad = []
    for combo, with_x, with_ln, p, with_dy, with_ds, with_dx in R.ADLN_COMBOS:
        what = f"rows={rows} D={D}{' misaligned' if misaligned else ''} {combo}"
        mask, s, y, mean, rstd = _Buf(n, fill=SENTINEL), _Buf(n), _Buf(n), _Buf(rows), _Buf(rows)
        _call("ast_add_drop_ln_fwd", _p(dev["x"]) if with_x else None, _p(sub), _p(mask) if p else None, _p(s), _p(dev["gamma"]) if with_ln else None,
              _p(dev["beta"]) if with_ln else None, _p(y) if with_ln else None, _p(mean) if with_ln else None, _p(rstd) if with_ln else None,
              rows, D, R.EPS, p, R.ADLN_SEED, _p(d_off))
        m64 = None
        if p:
            keep = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
            got = mask.t.cpu()
            assert bool(((got == 0) | (got == keep)).all()), f"{what}: the mask holds something other than 0 and 1 / (1 - p)"
            k = min(n, 512)
            assert torch.equal(got[:k], host_dropout_mask(R.ADLN_SEED, R.ADLN_OFFSET, k, p)), f"{what}: not the mask of ast_common.h"
            m64 = got.double().view(rows, D)
        else:
            assert bool((mask.t == SENTINEL).all())          # p = 0: no mask is written
        s64, y64, mu64, rs64 = R.add_drop_ln(i["x"] if with_x else None, i["sub"], m64, i["gamma"] if with_ln else None, i["beta"])
        p32 = _ln_plain32(i, m64, with_x, with_ln, with_dy, with_ds)
        bad += _close("add_drop_ln", f"{what} s", s.t, s64, p32["s"])
        if with_ln:
            bad += _close("add_drop_ln", f"{what} y", y.t, y64, p32["y"]) + _close("add_drop_ln", f"{what} mean", mean.t, mu64, p32["mean"])
            bad += _close("add_drop_ln", f"{what} rstd", rstd.t, rs64, p32["rstd"])
        else:
            assert bool(torch.isnan(y.t).all()) and bool(torch.isnan(mean.t).all())
        assert _intact(mask, s, y, mean, rstd, sub)
        dx64, dsub64, dg64, db64 = R.add_drop_ln_bwd(i["dy"] if with_dy else None, i["ds_ext"] if with_ds else None, s64,
                                                    i["gamma"], mu64, rs64, m64)
        # the size of the terms of rstd (g - mean(g) - xh mean(g xh)), for the one case where they cancel to exactly 0 (D = 1)
        terms = float(rs64.max() * (i["dy"] * i["gamma"]).abs().max()) if with_dy else None
        pg, pb = i["dgamma0"].float(), i["dbeta0"].float()
        runs = []
        for form in ("atomic", "det", "det"):
            dx, dsub, dg, db, ws = _Buf(n), _Buf(n, off=off), _Buf(D).from_(pg), _Buf(D).from_(pb), _Buf(2 * n)
            args = (_p(dev["dy"]) if with_dy else None, _p(dev["ds_ext"]) if with_ds else None, _p(s) if with_dy else None,
                    _p(dev["gamma"]) if with_dy else None, _p(mean) if with_dy else None, _p(rstd) if with_dy else None, _p(mask) if p else None,
                    _p(dx) if with_dx else None, _p(dsub), _p(dg), _p(db), rows, D)
            if form == "det":
                _call("ast_add_drop_ln_bwd_det", *args, _p(ws))
            else:
                _call("ast_add_drop_ln_bwd", *args)
            if with_dx:
                bad += _close("add_drop_ln", f"{what} dx {form}", dx.t, dx64, p32["dx"], terms=terms)
            else:
                assert bool(torch.isnan(dx.t).all())
            bad += _close("add_drop_ln", f"{what} dsub {form}", dsub.t, dsub64, p32["dsub"],
                          terms=None if terms is None else terms / (1.0 - p))
            if with_dy:
                bad += _close("add_drop_ln", f"{what} dgamma += {form}", dg.t, i["dgamma0"] + dg64, pg + p32["dgamma"])
                bad += _close("add_drop_ln", f"{what} dbeta += {form}", db.t, i["dbeta0"] + db64, pb + p32["dbeta"])
            else:
                assert torch.equal(dg.t.cpu(), pg) and torch.equal(db.t.cpu(), pb)
            assert _intact(dx, dsub, dg, db, ws)
            runs.append((dsub.t.cpu(), dg.t.cpu(), db.t.cpu()))
        assert all(torch.equal(a, b) for a, b in zip(runs[1], runs[2])), f"{what}: two deterministic runs differ"
    assert not bad, "\n".join(bad)
