"""The tail of a training step against the float64 references of tests/loss_tail_ref.py: the embedding losses, cross-entropy,
softmax entropy, ast_scale and the batch reconstruction loss of csrc/losses.hip, and the step scalars, sum of squares and Adam of
csrc/optim.hip -- through the C ABI and through ops / ast_amd, at the sizes where each kernel changes path (the case tables and
seeded inputs are loss_tail_ref's; tests/test_loss_tail_cpu.py checks the references, the conditions on the inputs and the launch
arithmetic below without a GPU).

Which loops the large cases enter (derived from the launch arithmetic, asserted in test_loss_tail_cpu.py):
  ast_sumsq, 256 workgroups x 256 threads, stride 65536 float4:
    n = 786436   thread 0 takes one 4-way unrolled trip, the other 65535 threads three single-stride trips
    n = 900001   28392 threads take one unrolled trip, the other 37144 three single-stride trips
    n = 1048583  every thread takes one unrolled trip, thread 0 one single-stride trip more
    n = 3000003  every thread takes up to three unrolled trips, 36432 of them up to three single-stride trips
    n <= 1027    at most one single-stride trip, no unrolled one; n = 1, 3: only the n & 3 tail
  ast_sumsq_det, `nslots` workgroups: 3000003 floats make 732 unrolled trips per thread at 1 slot, 46 at 16, 3 at 256
  ast_adam / ast_adam_dev / ast_scale, 4096 x 256 threads: n = 1048576 + 257 (+ 5) grid-strides, the smaller sizes do not
  ast_recon_loss, 256 workgroups x 1024 threads: (2, 2, 287, 513) has 294462 bins, so 32318 threads take a second bin
  ast_recon_loss_total, 256-thread workgroups capped at 65536: the cap needs more than 16.7 M bins per section, buffers of
    hundreds of MB, and is not reached here; at (2, 2, 287, 513) its 1151 workgroups share the 64 slots.

Tolerances are measured at run time, on the CPU (loss_tail_ref.bound): e32 is the error of the plain float32 evaluation (the float32
oracle, torch.nn.functional, torch.optim.Adam in float32) against float64 on the same inputs, and the kernel must be within
max(8 * e32, 64 * 2^-24 = 3.8e-6) of the float64 result, both relative to its max-abs.  What is exact by construction is compared
with torch.equal: ast_adam_dev against ast_adam, repeated calls, sentinels, zero gradients.  Every test prints its figures; the
worst per group on the MI355X (kernel error / e32 of that comparison / its bound):

  adam             2.7e-07 / 2.2e-07 / 3.8e-06      (p, m, v after each of the five steps)
  sumsq            4.4e-07 / 6.8e-09 / 3.8e-06
  sumsq_det        3.7e-07 / 3.0e-09 / 3.8e-06
  weighted_sum     4.9e-08 / 4.6e-08 / 3.8e-06
  scale            4.8e-08 / 4.8e-08 / 3.8e-06
  infonce          2.7e-06 / 8.4e-07 / 6.8e-06
  hsic             3.1e-06 / 2.9e-07 / 3.8e-06
  crosscov         7.8e-07 / 3.4e-07 / 3.8e-06
  margin           1.2e-07 / 1.2e-07 / 3.8e-06
  cross_entropy    below 0.13 of its bound everywhere (the worst ratio is a loss of 1e-26 that float32 rounds to 0: 1 / 1 / 8)
  softmax_entropy  5.1e-07 / 4.5e-07 / 3.8e-06
  recon_1024       4.4e-07 / 7.8e-08 / 3.8e-06      (ast_recon_loss)
  recon_total      3.1e-07 / 3.1e-07 / 3.8e-06      (ast_recon_loss_total)
  recon_route      3.1e-07 / 3.1e-07 / 3.8e-06      (compute_comprehensive_loss)

Two kernels missed the bound when these tests were first run and were changed (csrc/losses.hip):
  hsic_kernel formed the row means of K and L as sequential float32 sums and summed Kc * L.  The centred entries are ~0.03 where
    K is ~0.7, an error of a row mean enters a whole row with one sign, and the uncentred L multiplied it by B * mean(L): from
    B = 33 on the loss was 1.1e-5 ... 4.0e-5 and the gradients up to 1.0e-5 from float64 (float32 oracle: 2e-7).  The means are
    now summed in double and the loss is sum Kc * Lc.
  cross_entropy_kernel took the softmax of the gradient as exp(z - lse), which rounds at the size of the logits: 3.85e-6 at
    R = 257, C = 7, logits x50 (torch: 9.5e-8).  It is exp(z - max) / den now.
"""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_tail_ref as R
import recon_len_ref as RL
from oracle import ast_oracle as O

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import ast_amd
    from ast_amd import _lib, ops

DEV = "cuda"
GUARD = 64
SENTINEL = -24576.0
NAN = float("nan")
F64 = torch.float64
WORST = {}                # group -> (kernel error, e32, bound) of its worst comparison (largest error / bound)


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nworst comparison per group: kernel error / float32 floor e32 / bound")
    for g, (err, e32, tol) in sorted(WORST.items()):
        print(f"  {g:<22} {err:.2e} / {e32:.2e} / {tol:.2e}")


def _close(group, what, got, ref, plain32):
    """[] or one line of failure: got within the measured bound of the float64 ref; a ref that is all zero must be met exactly"""
    got, ref = torch.as_tensor(got).detach().cpu(), torch.as_tensor(ref).detach().cpu()
    assert got.numel() == ref.numel(), (what, tuple(got.shape), tuple(ref.shape))
    if not bool(torch.isfinite(got).all()):
        return [f"{what}: {int((~torch.isfinite(got)).sum())} of {got.numel()} values are not finite"]
    if R.is_zero(ref):
        return [] if float(got.abs().max()) == 0.0 else [f"{what}: the reference is exactly 0, the kernel gives up to {float(got.abs().max()):.3g}"]
    e32, tol = R.bound(plain32, ref)
    err = R.rel(got, ref)
    print(f"{group:<18} {what:<52} err {err:.2e}   e32 {e32:.2e}   bound {tol:.2e}")
    if group not in WORST or err / tol > WORST[group][0] / WORST[group][2]:
        WORST[group] = (err, e32, tol)
    return [] if err <= tol else [f"{what}: {err:.3g} of max|ref| from the float64 reference, bound {tol:.3g} (float32 evaluation: {e32:.3g})"]


class _Buf:
    """n elements between two sentinel bands, in one allocation."""

    def __init__(self, n, fill=NAN):
        self.all = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
        self.t = self.all[GUARD:GUARD + n]
        self.t.fill_(fill)

    def guards_intact(self):
        return bool((self.all[:GUARD] == SENTINEL).all()) and bool((self.all[-GUARD:] == SENTINEL).all())


def _call(name, *args):
    _lib.check(getattr(_lib.lib(), name)(*args, _lib.stream()), name)


def _dev(t):
    return t.to(DEV).contiguous()


# ---- ast_sumsq / ast_sumsq_det ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", R.SUMSQ_N)
def test_sumsq(n):
    if "AST_SUMSQ_BLOCKS" in os.environ:
        pytest.skip("AST_SUMSQ_BLOCKS is set: the workgroup cap is read once per process and the cases are built for its default, 256")
    x = R.sumsq_input(n)
    ref = R.sumsq(x)
    plain = float((x * x).sum())
    pre = R.f32(0.25 * ref + 1.0)                           # out is ADDED to
    xd = _dev(x)
    assert xd.data_ptr() % 16 == 0
    bad = []
    out = _Buf(1, pre)
    _call("ast_sumsq", _lib.ptr(xd), n, _lib.ptr(out.t))
    bad += _close("sumsq", f"ast_sumsq n={n}", out.t.cpu(), torch.tensor([pre + ref], dtype=F64), torch.tensor([np.float32(pre) + np.float32(plain)]))
    assert out.guards_intact()
    for slots in R.SUMSQ_SLOTS:
        out, ws = _Buf(1, pre), _Buf(slots)
        _call("ast_sumsq_det", _lib.ptr(xd), n, _lib.ptr(out.t), _lib.ptr(ws.t), slots)
        first = out.t.cpu().clone()
        bad += _close("sumsq_det", f"ast_sumsq_det n={n} slots={slots}", first, torch.tensor([pre + ref], dtype=F64),
                      torch.tensor([np.float32(pre) + np.float32(plain)]))
        assert out.guards_intact() and ws.guards_intact()
        out.t.fill_(pre)
        ws.t.fill_(NAN)
        _call("ast_sumsq_det", _lib.ptr(xd), n, _lib.ptr(out.t), _lib.ptr(ws.t), slots)
        if not torch.equal(out.t.cpu(), first):
            bad.append(f"ast_sumsq_det n={n} slots={slots}: two runs differ")
    assert not bad, "\n".join(bad)


# ---- ast_adam / ast_adam_dev ------------------------------------------------------------------------------------------------

def _adam_reference(n, wd, kind):
    """The float64 chain and torch.optim.Adam in float32 over the five steps of the test: counter 1, 2, 3, ADAM_BIG_STEP, then
    ADAM_BIG_STEP + 1 at half the learning rate.  -> [(step, lr, (p, m, v) float64, (p, m, v) float32)]"""
    h = R.ADAM_HYPER
    p0, g = R.adam_inputs(n)
    q, max_norm = R.adam_clip(kind, g)
    tp = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([tp], lr=R.f32(h["lr"]), betas=(R.f32(h["b1"]), R.f32(h["b2"])), eps=R.f32(h["eps"]), weight_decay=R.f32(wd))
    p, m, v = p0.double(), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    chain = []
    for step, lr in ((1, h["lr"]), (2, h["lr"]), (3, h["lr"]), (R.ADAM_BIG_STEP, h["lr"]), (R.ADAM_BIG_STEP + 1, 0.5 * h["lr"])):
        # the clip factor from the float32 gnorm_sq the kernel is handed, not from a float32 norm of torch's own (clip_grad_norm_'s
        # is 2.5e-5 off at a million elements, which would only widen the bound)
        tp.grad = g * np.float32(R.clip_factor(q, R.f32(max_norm)))
        if step == R.ADAM_BIG_STEP:
            opt.state[tp]["step"] = torch.tensor(float(step - 1))
        opt.param_groups[0]["lr"] = R.f32(lr)
        opt.step()
        p, m, v = R.adam_step(p, g, m, v, step, lr, h["b1"], h["b2"], h["eps"], wd, q, max_norm)
        st = opt.state[tp]
        chain.append((step, lr, (p, m, v), (tp.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone())))
    return chain


def _adam_run(n, wd, kind, on_device):
    """The same five steps on the GPU with ast_adam (host lr / max_norm) or ast_adam_dev ([lr, max_norm] written by ast_set_values)
    -> [(p, m, v)] after every step, on the host."""
    h = R.ADAM_HYPER
    p0, g = R.adam_inputs(n)
    q, max_norm = R.adam_clip(kind, g)
    p, gd, m, v = _Buf(n), _Buf(n), _Buf(n, 0.0), _Buf(n, 0.0)
    p.t.copy_(p0)
    gd.t.copy_(g)
    nrm = None if q is None else torch.tensor([q], dtype=torch.float32, device=DEV)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    hyper = _Buf(16)
    states = []
    for it in range(5):
        lr = h["lr"] if it < 4 else 0.5 * h["lr"]
        if it == 3:
            step.fill_(R.ADAM_BIG_STEP)
        else:
            _call("ast_counter_incr", _lib.ptr(step))
        if on_device:
            if it in (0, 4):                                # written once, then the learning rate changed ON THE DEVICE before the last step
                _call("ast_set_values", _lib.ptr(hyper.t), (C.c_float * 2)(lr, max_norm), 2)
            _call("ast_adam_dev", _lib.ptr(p.t), _lib.ptr(gd.t), _lib.ptr(m.t), _lib.ptr(v.t), n, _lib.ptr(hyper.t), h["b1"], h["b2"], h["eps"], wd,
                  _lib.ptr(step), _lib.ptr(nrm))
        else:
            _call("ast_adam", _lib.ptr(p.t), _lib.ptr(gd.t), _lib.ptr(m.t), _lib.ptr(v.t), n, lr, h["b1"], h["b2"], h["eps"], wd, _lib.ptr(step),
                  _lib.ptr(nrm), max_norm)
        states.append((p.t.cpu(), m.t.cpu(), v.t.cpu()))
    assert int(step) == R.ADAM_BIG_STEP + 1
    assert all(b.guards_intact() for b in (p, gd, m, v, hyper)) and torch.equal(gd.t.cpu(), g)
    return states


@pytest.mark.parametrize("n", R.ADAM_N)
def test_adam(n):
    bad = []
    for wd in R.ADAM_WD:
        runs = {}
        for kind in R.ADAM_CLIP:
            chain = _adam_reference(n, wd, kind)
            host, dev = _adam_run(n, wd, kind, False), _adam_run(n, wd, kind, True)
            runs[kind] = host
            for (step, lr, ref, plain), got, gotd in zip(chain, host, dev):
                for name, a, r, p32, ad in zip("pmv", got, ref, plain, gotd):
                    bad += _close("adam", f"ast_adam n={n} wd={wd} clip={kind} step={step} {name}", a, r, p32)
                    if not torch.equal(a, ad):
                        bad.append(f"n={n} wd={wd} clip={kind} step={step}: ast_adam_dev's {name} is not ast_adam's bit for bit")
        # a clip factor of exactly 1, however it comes about, is the unclipped update: the same bits
        for kind in ("null", "zero"):
            for s, (a, b) in enumerate(zip(runs["inactive"], runs[kind])):
                if not all(torch.equal(x, y) for x, y in zip(a, b)):
                    bad.append(f"n={n} wd={wd}: the inactive clip and clip={kind} differ at step index {s}")
        if all(torch.equal(x, y) for x, y in zip(runs["active"][0], runs["null"][0])):
            bad.append(f"n={n} wd={wd}: the active clip changed nothing")
    assert not bad, "\n".join(bad[:40])


# ---- ast_set_values / ast_weighted_sum / ast_weighted_sum_bwd -------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 5, 16])
def test_set_values(n):
    table = _Buf(16, SENTINEL)
    vals = [R.f32(0.37 * (i + 1) ** 2 - 3) for i in range(16)]
    _call("ast_set_values", _lib.ptr(table.t), (C.c_float * 16)(*vals), n)
    got = table.t.cpu()
    assert torch.equal(got[:n], torch.tensor(vals[:n], dtype=torch.float32))
    assert torch.equal(got[n:], torch.full((16 - n,), SENTINEL)) and table.guards_intact()


@pytest.mark.parametrize("n,widx", R.WSUM_CASES, ids=[f"n{c[0]}" for c in R.WSUM_CASES])
def test_weighted_sum(n, widx):
    terms, w = R.wsum_inputs(n)
    ref, wi = R.weighted_sum(terms, widx, w)
    s32 = np.float32(0)
    for a, t in zip(wi, terms):
        s32 = np.float32(s32 + np.float32(a) * np.float32(t))
    wd = _dev(w)
    td = [_dev(terms[i:i + 1].clone()) for i in range(n)]               # n distinct one-element tensors
    parr, iarr = (C.c_void_p * n)(*[t.data_ptr() for t in td]), (C.c_int32 * n)(*widx)
    bad, outs = [], []
    for _ in range(3):
        out = _Buf(1)
        _call("ast_weighted_sum", parr, iarr, n, _lib.ptr(wd), _lib.ptr(out.t))
        outs.append(out.t.cpu())
        assert out.guards_intact()
    bad += _close("weighted_sum", f"ast_weighted_sum n={n}", outs[0], torch.tensor([ref], dtype=F64), torch.tensor([s32]))
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    g = 1.7
    gd = torch.tensor([g], dtype=torch.float32, device=DEV)
    gref = torch.tensor([R.f32(g) * a for a in wi], dtype=F64)
    g32 = torch.tensor([np.float32(g) * np.float32(a) for a in wi])
    grads = _Buf(16, SENTINEL)
    _call("ast_weighted_sum_bwd", _lib.ptr(gd), iarr, n, _lib.ptr(wd), _lib.ptr(grads.t))
    got = grads.t.cpu()
    bad += _close("weighted_sum", f"ast_weighted_sum_bwd n={n}", got[:n], gref, g32)
    assert torch.equal(got[n:], torch.full((16 - n,), SENTINEL)) and grads.guards_intact()
    # ops.weighted_sum through autograd, a non-unit upstream gradient
    leaves = [t.reshape(()).clone().requires_grad_(True) for t in td]
    tot = [ops.weighted_sum(wd, list(zip(widx, leaves))) for _ in range(3)]
    assert torch.equal(tot[0].detach().cpu().reshape(1), outs[0]) and torch.equal(tot[0], tot[1]) and torch.equal(tot[0], tot[2])
    (tot[0] * g).backward()
    bad += _close("weighted_sum", f"ops.weighted_sum backward n={n}", torch.stack([l.grad for l in leaves]), gref, g32)
    assert not bad, "\n".join(bad)


# ---- InfoNCE --------------------------------------------------------------------------------------------------------------

def _infonce_case(what, s, lab, temp):
    kw = {} if temp is None else {"temperature": temp}
    t = 0.1 if temp is None else temp
    v64, g64 = R.with_grad(lambda a: R.infonce(a, lab, t), s)
    v32, g32 = R.with_grad(lambda a: O.infonce_loss(a, lab, t), s, dtype=torch.float32)
    sh = _dev(s).requires_grad_(True)
    loss = ast_amd.infoNCE_loss(sh, lab, **kw)
    loss.backward()
    return _close("infonce", what + " loss", loss, v64, v32) + _close("infonce", what + " grad", sh.grad, g64[0], g32[0])


@pytest.mark.parametrize("D", R.INFONCE_D)
@pytest.mark.parametrize("B", R.INFONCE_B)
def test_infonce(B, D):
    s, _ = R.embeddings(B, D)
    bad = []
    for layout in R.INFONCE_LAYOUTS:
        for temp in (None, 0.5):
            bad += _infonce_case(f"B={B} D={D} {layout} T={temp or 'default'}", s, R.labels(layout, B), temp)
    if (B, D) == (7, 100):                                  # the normalisation cancels the scale of the embeddings
        bad += _infonce_case("B=7 D=100 singleton x100", s * 100, R.labels("singleton", B), None)
    assert not bad, "\n".join(bad)


# ---- HSIC, cross-covariance, margin ----------------------------------------------------------------------------------------------

def _pair_case(group, what, s, c, fn64, fn32, use_hsic):
    v64, g64 = R.with_grad(fn64, s, c)
    v32, g32 = R.with_grad(fn32, s, c, dtype=torch.float32)
    sh, ch = _dev(s).requires_grad_(True), _dev(c).requires_grad_(True)
    loss = ast_amd.disentanglement_loss(sh, ch, use_hsic=use_hsic)
    loss.backward()
    return (_close(group, what + " loss", loss, v64, v32) + _close(group, what + " dstyle", sh.grad, g64[0], g32[0])
            + _close(group, what + " dcontent", ch.grad, g64[1], g32[1]))


@pytest.mark.parametrize("name,B,D,layout,seed", R.HSIC_CASES, ids=[c[0] for c in R.HSIC_CASES])
def test_hsic(name, B, D, layout, seed):
    s, c = R.hsic_inputs(B, D, layout, seed)
    bad = _pair_case("hsic", f"hsic {name}", s, c, R.hsic64, lambda a, b: O.disentanglement_loss(a, b), True)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("D", R.EMB_D)
@pytest.mark.parametrize("B", R.CROSSCOV_B)
def test_crosscov(B, D):
    s, c = R.embeddings(B, D)
    bad = _pair_case("crosscov", f"crosscov B={B} D={D}", s, c, R.crosscov, R.crosscov, False)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("Cn,D", R.MARGIN_CASES)
def test_margin(Cn, D):
    cls = R.margin_rows(Cn, D)
    v64, g64 = R.with_grad(lambda a: R.margin(a, R.MARGIN), cls)
    v32, g32 = R.with_grad(lambda a: R.margin(a, R.MARGIN), cls, dtype=torch.float32)
    ch = _dev(cls).requires_grad_(True)
    loss = ast_amd.margin_loss(ch, margin=R.MARGIN)
    loss.backward()
    bad = _close("margin", f"margin C={Cn} D={D} loss", loss, v64, v32) + _close("margin", f"margin C={Cn} D={D} grad", ch.grad, g64[0], g32[0])
    if (Cn, D) == (2, 256):
        assert R.is_zero(g64[0]) and torch.equal(ch.grad.cpu(), torch.zeros(Cn, D))
    assert not bad, "\n".join(bad)


# ---- cross-entropy, softmax entropy -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Cn", R.ROW_C)
@pytest.mark.parametrize("Rn", R.ROW_R)
def test_cross_entropy_and_softmax_entropy(Rn, Cn):
    bad = []
    up = 1.7                                                # a non-unit upstream gradient: the backward is one ast_scale launch
    for sc in R.ROW_SCALE:
        z, t = R.row_inputs(Rn, Cn, sc)
        for name, fn64, fn32, run in (
                ("cross_entropy", lambda a: R.cross_entropy(a, t), lambda a: F.cross_entropy(a, t.long()),
                 lambda zh: ops.CrossEntropyFn.apply(zh, _dev(t))),
                ("softmax_entropy", R.softmax_entropy, R.softmax_entropy, lambda zh: ops.SoftmaxEntropyFn.apply(zh))):
            v64, g64 = R.with_grad(fn64, z)
            v32, g32 = R.with_grad(fn32, z, dtype=torch.float32)
            zh = _dev(z).requires_grad_(True)
            loss = run(zh)
            (loss * up).backward()
            what = f"{name} R={Rn} C={Cn} x{sc:g}"
            bad += _close(name, what + " loss", loss, v64, v32) + _close(name, what + " grad", zh.grad, R.f32(up) * g64[0], np.float32(up) * g32[0])
    assert not bad, "\n".join(bad)


# ---- ast_scale -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", R.SCALE_N)
def test_scale(n):
    g = torch.Generator().manual_seed(12000 + n % 9973)
    x, y0 = torch.randn(n, generator=g), torch.randn(n, generator=g)
    hs, ds = 0.75, torch.tensor([-1.3], dtype=torch.float32)
    xd, dsd = _dev(x), _dev(ds)
    bad = []
    for acc in (0, 1):
        for dscale in (None, ds):
            y = _Buf(n)
            y.t.copy_(y0)
            _call("ast_scale", _lib.ptr(xd), None if dscale is None else _lib.ptr(dsd), hs, _lib.ptr(y.t), n, acc)
            sc32 = np.float32(hs) * (np.float32(1) if dscale is None else dscale.numpy()[0])
            plain = y0 + float(sc32) * x if acc else float(sc32) * x
            bad += _close("scale", f"ast_scale n={n} accumulate={acc} dscale={'device' if dscale is not None else 'NULL'}", y.t,
                          R.scale(x, y0, hs, None if dscale is None else ds[0], acc), plain)
            assert y.guards_intact()
    y = _Buf(n)
    y.t.copy_(y0)
    _call("ast_scale", _lib.ptr(y.t), None, 0.5, _lib.ptr(y.t), n, 0)  # in place, as the trainer averages gradients: a power of two is exact
    assert torch.equal(y.t.cpu(), 0.5 * y0) and y.guards_intact()
    assert not bad, "\n".join(bad)


# ---- the batch reconstruction loss ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _recon(name):
    """Inputs and references of a case, computed once: float64 and plain float32 (sums, total, grad) at the float32 coefficients."""
    _, B, S, T, Fq, ld, phases = next(c for c in R.RECON_CASES if c[0] == name)
    out, x = R.recon_inputs(B, S, T, Fq, ld, phases)
    coef, inv = R.recon_coefs(B, S, T, Fq)
    coef, inv = tuple(R.f32(c) for c in coef), tuple(R.f32(c) for c in inv)
    ref = RL.recon_batch_ref(out, x[..., :Fq], coef)
    plain = RL.recon_batch_ref(out, x[..., :Fq], coef, dtype=torch.float32)
    return (B, S, T, Fq, ld), out, x, coef, inv, ref, plain


RECON_IDS = [c[0] for c in R.RECON_CASES]


def _close_sums(group, what, got5, ref5, plain5):
    """the five sums one by one (their sizes differ by orders of magnitude); a term without elements is exactly 0"""
    bad = []
    for k, key in enumerate(RL.KEYS):
        bad += _close(group, f"{what} {key}", got5[k:k + 1], ref5[k:k + 1], plain5[k:k + 1])
    return bad


@pytest.mark.parametrize("name", RECON_IDS)
def test_recon_loss_1024(name):
    """ast_recon_loss: 1024-thread workgroups, at most 256 of them, partial sums added with atomics into one row."""
    (B, S, T, Fq, ld), out, x, coef, inv, ref, plain = _recon(name)
    od, xd = _dev(out), _dev(x)
    sums, grad = _Buf(5), _Buf(out.numel())
    _call("ast_recon_loss", _lib.ptr(od), _lib.ptr(xd), ld, B, S, T, Fq, *coef, _lib.ptr(sums.t), _lib.ptr(grad.t))
    bad = _close_sums("recon_1024", f"ast_recon_loss {name}", sums.t.cpu(), ref[0], plain[0])
    bad += _close("recon_1024", f"ast_recon_loss {name} grad", grad.t, ref[2], plain[2])
    assert sums.guards_intact() and grad.guards_intact()
    sums2 = _Buf(5)
    _call("ast_recon_loss", _lib.ptr(od), _lib.ptr(xd), ld, B, S, T, Fq, *coef, _lib.ptr(sums2.t), None)         # values only
    bad += _close_sums("recon_1024", f"ast_recon_loss {name} (no grad)", sums2.t.cpu(), ref[0], plain[0])
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("with_grad", [True, False], ids=["grad", "values"])
@pytest.mark.parametrize("name", RECON_IDS)
def test_recon_loss_total(name, with_grad):
    (B, S, T, Fq, ld), out, x, coef, inv, ref, plain = _recon(name)
    od, xd = _dev(out), _dev(x)
    ws, res, grad = _Buf(64 * 5), _Buf(11), _Buf(out.numel())
    _call("ast_recon_loss_total", _lib.ptr(od), _lib.ptr(xd), ld, B, S, T, Fq, (C.c_float * 5)(*coef), (C.c_float * 5)(*inv), _lib.ptr(ws.t),
          _lib.ptr(res.t), _lib.ptr(grad.t) if with_grad else None)
    got = res.t.cpu()
    i64, i32 = torch.tensor(inv, dtype=F64), torch.tensor(inv, dtype=torch.float32)
    bad = _close_sums("recon_total", f"ast_recon_loss_total {name} sum", got[:5], ref[0], plain[0])
    bad += _close_sums("recon_total", f"ast_recon_loss_total {name} mean", got[6:], ref[0] * i64, plain[0] * i32)
    bad += _close("recon_total", f"ast_recon_loss_total {name} total", got[5:6], ref[1], plain[1])
    if with_grad:
        bad += _close("recon_total", f"ast_recon_loss_total {name} grad", grad.t, ref[2], plain[2])
    else:
        assert bool(torch.isnan(grad.t).all())
    assert ws.guards_intact() and res.guards_intact() and grad.guards_intact()
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", RECON_IDS)
def test_compute_comprehensive_loss(name):
    """The route of the training step: new_decoder.compute_comprehensive_loss -> ops.ReconTotalFn -> ast_recon_loss_total, the
    target a [..., :Fq] slice, the gradient scaled by a non-unit upstream factor (ast_scale)."""
    (B, S, T, Fq, ld), out, x, coef, inv, ref, plain = _recon(name)
    oh = _dev(out).requires_grad_(True)
    got = ast_amd.compute_comprehensive_loss(oh, x.to(DEV)[..., :Fq])
    up = 1.7
    (got["total_loss"] * up).backward()
    i64, i32 = torch.tensor(inv, dtype=F64), torch.tensor(inv, dtype=torch.float32)
    bad = _close("recon_route", f"compute_comprehensive_loss {name} total", got["total_loss"], ref[1], plain[1])
    for k, key in enumerate(RL.KEYS):
        bad += _close("recon_route", f"compute_comprehensive_loss {name} {key}", got[key], (ref[0] * i64)[k], (plain[0] * i32)[k])
    bad += _close("recon_route", f"compute_comprehensive_loss {name} grad", oh.grad, R.f32(up) * ref[2], np.float32(up) * plain[2])
    assert not bad, "\n".join(bad)
