"""Host side of the loss / optimiser tail tests (no GPU): the float64 references of tests/loss_tail_ref.py against the float32
oracle, torch.nn.functional, torch.optim.Adam in double and tests/golden/losses.npz; the conditions the seeded inputs of every
GPU case must meet for the comparison to mean something (section "cases and seeded inputs" of loss_tail_ref.py); the launch
arithmetic that says which loops each large case enters; and the argument refusals of ast_margin, ast_hsic and ast_crosscov."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_tail_ref as R
import recon_len_ref as RL
from oracle import ast_oracle as O
from oracle import seeded_params as sp

F64 = torch.float64


def _golden_inputs(B):
    rng = np.random.default_rng([77, B])
    style = torch.tensor(rng.standard_normal((B, 256)).astype(np.float32))
    content = torch.tensor(rng.standard_normal((B, 3, 256)).astype(np.float32))
    return style, content


# ---- the references themselves -------------------------------------------------------------------------------------------

def test_oracle_functions_stay_in_float64():
    """What loss_tail_ref takes from the oracle is float64 end to end: the result is float64 and differs from the float32
    evaluation by float32 rounding, not by nothing (a hidden .float() would make the two agree to the last bit)."""
    s, c = R.embeddings(8, 100)
    lab = R.labels("balanced", 8)
    out, x = R.recon_inputs(2, 2, 5, 7, 7, "random")
    cases = {"infonce": lambda t: O.infonce_loss(s.to(t), lab), "margin": lambda t: O.margin_loss(s[:3].to(t) * 0.05),
             "crosscov": lambda t: O.disentanglement_loss(s.to(t), c.to(t), use_hsic=False),
             "comprehensive": lambda t: O.comprehensive_loss(out.to(t), x.to(t))["total_loss"]}
    for name, fn in cases.items():
        v64, v32 = fn(F64), fn(torch.float32)
        assert v64.dtype == F64 and v32.dtype == torch.float32, name
        d = abs(float(v64) - float(v32)) / abs(float(v64))
        assert 0 < d < 1e-5, (name, d)
    with pytest.raises(RuntimeError):                      # the HSIC branch mixes a float32 eye into float64: hence hsic64
        O.disentanglement_loss(s.double(), c.double(), use_hsic=True)


@pytest.mark.parametrize("B", [8, 16])
def test_embedding_references_match_golden(golden_dir, B):
    g = np.load(os.path.join(golden_dir, "losses.npz"))
    style, content = _golden_inputs(B)
    lab = sp.balanced_labels(B)
    cm = content.mean(1)
    for name, fn, xs, keys in (
            ("infonce", lambda s: R.infonce(s, lab), (style,), ("dstyle",)),
            ("hsic", R.hsic64, (style, cm), ("dstyle",)),
            ("crosscov", R.crosscov, (style, cm), ("dstyle",))):
        v, gs = R.with_grad(fn, *xs)
        assert math.isclose(float(v), float(g[f"B{B}_{name}"]), rel_tol=2e-5), name
        assert R.rel(gs[0], torch.tensor(g[f"B{B}_{name}_dstyle"])) < 2e-5, name
    # hsic: the content gradient through the section mean
    c3 = content.double().requires_grad_(True)
    R.hsic64(style.double(), c3.mean(1)).backward()
    assert R.rel(c3.grad, torch.tensor(g[f"B{B}_hsic_dcontent"])) < 2e-5


@pytest.mark.parametrize("name,B,D,layout,seed", R.HSIC_CASES, ids=[c[0] for c in R.HSIC_CASES])
def test_hsic_reference_matches_float32_oracle_and_median_is_isolated(name, B, D, layout, seed):
    s, c = R.hsic_inputs(B, D, layout, seed)
    assert R.hsic_rank(B) == O.hsic_sigma_rank(B)
    gap = R.hsic_median_gap(s, c)
    print(f"hsic {name}: relative gap at the median {gap:.2e}")
    assert gap > R.HSIC_GAP, f"{name}: the median distance is {gap:.2e} (relative) from another pair's: choose another seed"
    if B <= 64:
        v64, g64 = R.with_grad(R.hsic64, s, c)
        v32, g32 = R.with_grad(lambda a, b: O.disentanglement_loss(a, b), s, c, dtype=torch.float32)
        assert R.rel(v32, v64) < 1e-4 and R.rel(g32[0], g64[0]) < 1e-3 and R.rel(g32[1], g64[1]) < 1e-3


def test_row_loss_references_match_torch():
    for R_ in R.ROW_R:
        for C in R.ROW_C:
            for sc in R.ROW_SCALE:
                z, t = R.row_inputs(R_, C, sc)
                assert (int(t.min()) == 0 or R_ == 1) and int(t.max()) == C - 1 and int(t[-1]) == C - 1     # one row: one target, C - 1
                z64 = z.double()
                ce = R.cross_entropy(z64, t)
                ref = F.cross_entropy(z.double(), t.long())
                assert abs(float(ce) - float(ref)) <= 1e-13 * max(1.0, abs(float(ref)))
                assert abs(float(ce) - float(O._cross_entropy(z, t.long()))) <= 1e-5 * max(1.0, abs(float(ref)))
                p = torch.softmax(z.double(), -1)
                ent = R.softmax_entropy(z64)
                assert abs(float(ent) - float(-(p * torch.log(p + 1e-8)).sum(-1).mean())) <= 1e-14
                p32 = torch.softmax(z, -1)
                assert abs(float(ent) - float(-(p32 * torch.log(p32 + 1e-8)).sum(-1).mean())) <= 1e-5
    # known answer: uniform logits -> -log(1/C + 1e-8)
    assert math.isclose(float(R.softmax_entropy(torch.zeros(5, 7, dtype=F64))), -math.log(1 / 7 + 1e-8), rel_tol=1e-14)


@pytest.mark.parametrize("wd", R.ADAM_WD)
def test_adam_reference_matches_torch_adam_in_double(wd):
    """Four steps with an active clip (clip_grad_norm_ first; torch's weight_decay also adds wd * p to the clipped gradient)."""
    h = {k: R.f32(v) for k, v in R.ADAM_HYPER.items()}
    p0, g = R.adam_inputs(255)
    q, max_norm = R.adam_clip("active", g)
    tp = p0.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([tp], lr=h["lr"], betas=(h["b1"], h["b2"]), eps=h["eps"], weight_decay=R.f32(wd))
    p, m, v = p0.double(), torch.zeros(255, dtype=F64), torch.zeros(255, dtype=F64)
    for step in (1, 2, 3, 4):
        tp.grad = g.double().clone()
        torch.nn.utils.clip_grad_norm_([tp], max_norm)
        opt.step()
        p, m, v = R.adam_step(p, g, m, v, step, wd=wd, gnorm_sq=R.sumsq(g), max_norm=max_norm, **R.ADAM_HYPER)
        st = opt.state[tp]
        assert R.rel(p, tp) < 1e-13 and R.rel(m, st["exp_avg"]) < 1e-12 and R.rel(v, st["exp_avg_sq"]) < 1e-12
    assert R.clip_factor(q, max_norm) < 0.03 and R.clip_factor(*R.adam_clip("inactive", g)) == 1.0
    assert R.clip_factor(None, 1.0) == 1.0 and R.clip_factor(q, 0.0) == 1.0


def test_recon_batch_reference_matches_oracle_and_per_clip_reference():
    for name, B, S, T, Fq, ld, phases in R.RECON_CASES:
        if B * T * Fq > 100000:
            B, S, T, Fq, ld = 2, 2, 9, 13, 13                # the same generator at a size the host checks in no time
        out, x = R.recon_inputs(B, S, T, Fq, ld, phases)
        tgt = x[..., :Fq]
        coef, inv = R.recon_coefs(B, S, T, Fq)
        sums, total, grad = RL.recon_batch_ref(out, tgt, coef)
        rows = RL.recon_len_ref(out.numpy(), tgt.numpy())
        assert np.allclose(sums.numpy(), rows[:, :5].sum(0), rtol=1e-12, atol=0), name
        if T > 1:
            o = out.double().requires_grad_(True)
            ref = O.comprehensive_loss(o, tgt.double())
            ref["total_loss"].backward()
            assert math.isclose(float(total), float(ref["total_loss"].detach()), rel_tol=1e-12), name
            assert R.rel(grad, o.grad) < 1e-12, name
            for k, key in enumerate(RL.KEYS):
                assert math.isclose(float(sums[k]) * inv[k], float(ref[key].detach()), rel_tol=1e-12, abs_tol=1e-300), (name, key)


def test_weighted_sum_and_scale_references():
    for n, widx in R.WSUM_CASES:
        terms, w = R.wsum_inputs(n)
        v, ws = R.weighted_sum(terms, widx, w)
        ref = sum((1.0 if i < 0 else float(w[i])) * float(t) for i, t in zip(widx, terms))
        assert math.isclose(v, ref, rel_tol=1e-14) and len(ws) == n == len(widx)
        assert len(set(terms.tolist())) == n and len(set(w.tolist())) == 16
    allw = [i for _, widx in R.WSUM_CASES for i in widx]
    assert -1 in allw and 15 in allw and any(allw.count(i) > 1 for i in set(allw) if i >= 0)
    x, y = torch.randn(7), torch.randn(7)
    assert torch.equal(R.scale(x, y, 0.5, torch.tensor(3.0), 1), y.double() + 1.5 * x.double())
    assert torch.equal(R.scale(x, y, 0.5, None, 0), 0.5 * x.double())


# ---- conditions on the inputs of every GPU case --------------------------------------------------------------------------

def test_infonce_inputs():
    for B in R.INFONCE_B:
        for D in R.INFONCE_D:
            s, _ = R.embeddings(B, D)
            assert float(s.norm(dim=1).min()) > 1.0, (B, D)             # no zero row
        for layout in R.INFONCE_LAYOUTS:
            lab = R.labels(layout, B)
            cnt = (lab[:, None] == lab[None, :]).sum(1) - 1
            assert lab.shape == (B,)
            if layout == "singleton" and B >= 3:
                assert int((cnt == 0).sum()) == 1 and int(cnt[0]) == 0, (layout, B)
            if layout == "one-class":
                assert int(cnt.min()) == B - 1
            if layout == "distinct" or B == 2 and layout != "one-class":
                assert int(cnt.max()) == 0
            if layout == "balanced" and B >= 4:
                assert int(cnt.min()) >= 1


def test_margin_inputs_cover_the_branches():
    tot = np.zeros(3, dtype=int)
    for C, D in R.MARGIN_CASES:
        cls = R.margin_rows(C, D)
        assert cls.shape == (C, D)
        tot += np.array(R.margin_pairs(cls))
    assert (tot > 0).all(), tot                            # pairs inside the margin, pairs outside, a pair of identical rows
    assert R.margin_pairs(R.margin_rows(2, 256)) == (0, 1, 0)           # the case whose gradient is exactly zero
    assert R.margin_pairs(R.margin_rows(3, 256))[2] == 1 and R.margin_pairs(R.margin_rows(5, 100))[2] == 1


@pytest.mark.parametrize("case", R.RECON_CASES, ids=[c[0] for c in R.RECON_CASES])
def test_recon_inputs(case):
    name, B, S, T, Fq, ld, phases = case
    out, x = R.recon_inputs(B, S, T, Fq, ld, phases)
    assert tuple(out.shape) == (B, S, 2, T, Fq) and tuple(x.shape) == (B, S, 2, T, ld)
    mag = torch.sqrt(out[:, :, 0].double() ** 2 + out[:, :, 1].double() ** 2)
    assert float(mag.min()) >= R.RECON_MIN_MAG
    d = R.wrapped_phase_difference(out, x[..., :Fq])
    assert float((math.pi - d.abs()).min()) > R.RECON_PHASE_GUARD
    raw = torch.atan2(out[:, :, 1], out[:, :, 0]).double() - torch.atan2(x[..., :Fq][:, :, 1], x[..., :Fq][:, :, 0]).double()
    if phases == "cut":                                     # every raw difference is about -+2 pi, every wrapped one about +-0.1
        assert float(raw.abs().min()) > 2 * math.pi - 0.2 and float(d.abs().max()) < 0.2
        assert bool((raw > 0).any()) and bool((raw < 0).any())
    elif B * S * T * Fq > 30:
        assert bool((raw > math.pi).any()) and bool((raw < -math.pi).any())


def test_sumsq_and_adam_inputs_and_launch_arithmetic():
    """Which loops of sumsq_kernel the cases enter, from the launch arithmetic (grid = min(n/4/256 + 1, 256) workgroups of 256;
    a thread enters the 4-way unrolled loop while i + 3 * stride < n / 4 and the single-stride loop for what is left)."""
    loops = {n: R.sumsq_loops(n, R.sumsq_grid(n)) for n in R.SUMSQ_N}
    for n in (1, 3, 4, 1027):
        assert loops[n][0] == 0 and loops[n][3] <= 1
    assert loops[1] == loops[3] == (0, 0, 0, 0)                         # n4 = 0: only the n & 3 tail
    assert R.sumsq_grid(786432) == 256 and R.sumsq_loops(786432, 256)[0] == 0      # the unrolled loop first runs just past here
    assert loops[786436] == (1, 1, 65535, 3)                # one thread takes one unrolled trip, the others three single strides
    u, ut, r, rt = loops[900001]
    assert 0 < u < 65536 and ut == 1 and r == 65536 - u and rt == 3         # unrolled for some threads, three single strides for the others
    assert loops[1048583] == (65536, 1, 1, 1)               # every thread takes one unrolled trip, thread 0 one more single stride
    assert loops[3000003][1] == 3 and loops[3000003][0] == 65536 and loops[3000003][2] > 0          # several unrolled trips
    for slots in R.SUMSQ_SLOTS:                             # ast_sumsq_det: the grid is the slot count
        assert R.sumsq_loops(3000003, slots)[1] >= 3
    # ast_adam / ast_scale: 4096 workgroups of 256; only the last size of each strides
    assert [n > 4096 * 256 for n in R.ADAM_N] == [False, False, False, True]
    assert [n > 4096 * 256 for n in R.SCALE_N] == [False, True]
    for n in R.ADAM_N:
        p, g = R.adam_inputs(n)
        q, mx = R.adam_clip("active", g)
        assert math.isclose(math.sqrt(q) / mx, 50, rel_tol=1e-3) and math.isclose(math.sqrt(q) / R.adam_clip("inactive", g)[1], 0.1, rel_tol=1e-3)
    x = R.sumsq_input(3000003)
    assert float(x.abs().min()) >= 0 and len(torch.unique(x[:4096] ** 2)) == 4096
    # ast_recon_loss: 1024-thread workgroups capped at 256
    name, B, S, T, Fq, ld, _ = R.RECON_CASES[0]
    assert B * T * Fq == 294462 > 256 * 1024


# ---- argument refusals settled with these tests --------------------------------------------------------------------------

def test_embedding_loss_entries_refuse_what_their_kernels_cannot_do():
    """ast_margin checks D; ast_hsic / ast_crosscov write both gradients or none, so one without the other is refused (it used to
    return the loss and leave the one gradient buffer unwritten).  Refused on the host: the fake pointers are never read."""
    from ast_amd import _lib
    lib = _lib.lib()
    fake = 0x10000
    assert lib.ast_margin(fake, 2, 0, 2.0, fake, fake, None) != 0 and b"ast_margin" in lib.ast_last_error()
    assert lib.ast_margin(fake, 2, -3, 2.0, fake, None, None) != 0 and lib.ast_margin(fake, 1, 8, 2.0, fake, None, None) != 0
    for fn, name in ((lib.ast_hsic, b"ast_hsic"), (lib.ast_crosscov, b"ast_crosscov")):
        assert fn(fake, fake, 4, 8, fake, fake, None, fake, None) != 0 and name in lib.ast_last_error()
        assert b"together" in lib.ast_last_error()
        assert fn(fake, fake, 4, 8, fake, None, fake, fake, None) != 0
        assert fn(fake, fake, 4, 0, fake, fake, fake, fake, None) != 0
        assert fn(fake, fake, 1, 8, fake, fake, fake, fake, None) != 0
