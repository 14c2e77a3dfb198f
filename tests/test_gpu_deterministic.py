"""Deterministic mode (ast_amd.set_deterministic, TrainConfig.deterministic): the train step repeats BIT FOR BIT.

Two Trainers with the same seed, config and input (dropout off) must give torch.equal losses, parameters, Adam moments and
module buffers (BatchNorm running statistics, spectral-norm u / v) after every step, in every execution mode and both compute
dtypes; the execution modes must agree with each other bitwise; the deterministic step must compute the default step (noise
model of test_gpu_trainer.py); and no entry point outside the deterministic forms may be called."""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import ast_amd
    from ast_amd import _lib, config, ops, train

MODES = {                                    # (use_graph, multi_stream, segmented)
    "eager_1stream": (False, False, False),
    "eager_streams": (False, True, False),
    "one_graph": (True, True, False),
    "segmented": (True, True, True),
}


def _state(tr):
    ts = {"G.flat_p": tr.G.flat_p, "G.m": tr.G.m, "G.v": tr.G.v, "D.flat_p": tr.D.flat_p, "D.m": tr.D.m, "D.v": tr.D.v}
    for tag, m in (("style", tr.style), ("content", tr.content), ("decoder", tr.decoder), ("disc", tr.disc)):
        for n, b in m.named_buffers():
            ts[f"{tag}.{n}"] = b
    return {k: v.detach().clone() for k, v in ts.items()}


def _run(mode, dtype, steps=3, deterministic=True, decoder="new"):
    use_graph, multi_stream, segmented = MODES[mode]
    ast_amd.set_compute_dtype(dtype)
    try:
        tr = train.Trainer(train.TrainConfig(use_graph=use_graph, multi_stream=multi_stream, segmented=segmented, dropout=False,
                                             deterministic=deterministic, decoder=decoder), seed=7)
        x, labels = train.synthetic_batch(4, 1, "cuda:0", seed=3)
        hist = []
        for _ in range(steps):
            out = tr.step(x, labels)
            torch.cuda.synchronize()
            hist.append(({k: v.detach().clone() for k, v in out.items()}, _state(tr)))
        return hist
    finally:
        ast_amd.set_compute_dtype(torch.float32)


def _assert_equal_hist(a, b, what):
    assert len(a) == len(b)
    for i, ((la, sa), (lb, sb)) in enumerate(zip(a, b)):
        assert la.keys() == lb.keys()
        for k in la:
            assert torch.equal(la[k], lb[k]), (what, i, k, float(la[k]), float(lb[k]))
        for k in sa:
            if not torch.equal(sa[k], sb[k]):
                d = (sa[k].double() - sb[k].double()).abs().max()
                raise AssertionError(f"{what}: step {i}: {k} differs (max abs {float(d):.3e})")


_REF = {}


def _ref(dtype):
    if dtype not in _REF:
        _REF[dtype] = _run("eager_1stream", dtype)
    return _REF[dtype]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("mode", list(MODES))
def test_deterministic_trainer_repeats_bitwise(mode, dtype):
    dt = torch.float32 if dtype == "f32" else torch.bfloat16
    a = _run(mode, dt)
    b = _run(mode, dt)
    _assert_equal_hist(a, b, (mode, dtype, "run to run"))
    assert all(math.isfinite(float(v)) for l, _ in a for v in l.values())
    assert float(a[0][0]["total"]) != float(a[-1][0]["total"])       # the optimiser moves the weights
    # mode independence: every execution mode computes the eager single-stream step bit for bit
    _assert_equal_hist(a, _ref(dt), (mode, dtype, "against eager single-stream"))


@pytest.mark.parametrize("mode", ["eager_1stream", "one_graph"])
def test_deterministic_simple_decoder_repeats_bitwise(mode):
    """decoder="simple" (SimpleDecoder_TransformerOnly): its two huge linears through per-chunk slabs (ast_bigk_gemm_det,
    ast_bign_dgrad_det); f32, the graph mode against eager single-stream as well."""
    a = _run(mode, torch.float32, decoder="simple")
    b = _run(mode, torch.float32, decoder="simple")
    _assert_equal_hist(a, b, (mode, "simple", "run to run"))
    assert float(a[0][0]["total"]) != float(a[-1][0]["total"])
    if mode != "eager_1stream":
        _assert_equal_hist(a, _run("eager_1stream", torch.float32, decoder="simple"), (mode, "simple", "against eager single-stream"))


def test_default_and_deterministic_compute_the_same_step():
    from test_gpu_trainer import _noise_tolerances, _run as _run_default, _assert_close_hist
    ref = _run_default(False, False)[0]
    ref2 = _run_default(False, False)[0]
    tols = _noise_tolerances(ref, ref2)
    det = [{k: float(v) for k, v in l.items()} for l, _ in _run("eager_1stream", torch.float32)]
    _assert_close_hist(det, ref, tols, "deterministic vs default")


# ---- the step launches only deterministic forms ------------------------------------------------------------------------------
# ALLOW-LIST: the entry points a deterministic step may call.  None of their kernels adds floats into global memory with atomics
# (the *_det forms, ast_wgrad_slab / ast_slab_sum, igemm with flags bit 12; the rest reduce within a workgroup or write each
# element from one thread).  Anything else -- a new entry point included -- fails the test until it is checked and listed here.
_ALLOWED = {
    "ast_version", "ast_last_error", "ast_igemm_plan", "ast_igemm_ws_floats_det", "ast_sn_scratch_floats",
    "ast_ordered_sum", "ast_sumsq_det", "ast_colsum_acc_det", "ast_chan_stats_det", "ast_norm_bwd_sums_det", "ast_layernorm_bwd_det",
    "ast_add_drop_ln_bwd_det", "ast_recon_loss_total_det", "ast_weight_grads_flush_det", "ast_bigk_gemm_det", "ast_bign_dgrad_det",
    "ast_bigk_gemm_det_ws_floats", "ast_bign_dgrad_det_ws_floats", "ast_wgrad_slab", "ast_slab_sum",
    "ast_igemm",                                   # only with flags bit 12, checked below
    "ast_weights_prepare_t", "ast_skinny_gemm", "ast_skinny_gemm_ex", "ast_linear_wgrad", "ast_linear_wgrad_batched_host",
    "ast_attn_fwd_p", "ast_attn_bwd_p", "ast_layernorm_fwd", "ast_add_drop_ln_fwd", "ast_norm_finalize", "ast_affine_act",
    "ast_norm_bwd_finalize", "ast_norm_bwd_apply_pre", "ast_nchw_to_nhwc", "ast_nhwc_to_nchw", "ast_cast", "ast_adaptive_pool_fwd",
    "ast_adaptive_pool_bwd", "ast_bilinear_fwd", "ast_bilinear_bwd", "ast_rowmix", "ast_mul", "ast_add", "ast_relu_bwd",
    "ast_dropout_fwd", "ast_dropout_mask", "ast_scale", "ast_weighted_sum", "ast_weighted_sum_bwd", "ast_infonce", "ast_margin",
    "ast_hsic", "ast_crosscov", "ast_cross_entropy", "ast_softmax_entropy", "ast_counter_incr", "ast_adam_dev", "ast_set_values",
}


class _Recorder:
    def __init__(self, raw):
        self.raw, self.calls = raw, []

    def __getattr__(self, name):
        fn = getattr(self.raw, name)
        if not name.startswith("ast_"):
            return fn

        def rec(*args):
            self.calls.append((name, args))
            return fn(*args)
        return rec


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_deterministic_step_calls_only_deterministic_forms(dtype):
    ast_amd.set_compute_dtype(dtype)
    tr = train.Trainer(train.TrainConfig(use_graph=False, multi_stream=False, dropout=False, deterministic=True), seed=7)
    x, labels = train.synthetic_batch(4, 1, "cuda:0", seed=3)
    raw = _lib.lib()
    rec = _Recorder(raw)
    _lib._lib = rec
    try:
        tr.step(x, labels)
        torch.cuda.synchronize()
    finally:
        _lib._lib = raw
        ast_amd.set_compute_dtype(torch.float32)
    names = {n for n, _ in rec.calls}
    assert names, "the recorder saw no calls"
    assert names <= _ALLOWED, sorted(names - _ALLOWED)
    for n, args in rec.calls:
        if n == "ast_igemm":
            assert args[6] & 4096 and not (args[6] & (8 | 16 | 64)), (n, args[6])   # the atomic-free instantiations only
    assert "ast_wgrad_slab" in names and "ast_sumsq_det" in names and "ast_recon_loss_total_det" in names
    # no ATen op on the path is flagged as nondeterministic
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    ast_amd.set_compute_dtype(dtype)
    try:
        tr.step(x, labels)
        torch.cuda.synchronize()
    finally:
        torch.use_deterministic_algorithms(prev)
        ast_amd.set_compute_dtype(torch.float32)


# ---- kernel level: the deterministic entry points repeat bitwise across streams and match a float64 reference -------------
def _three_calls(fn, outs):
    """fn() three times -- on the current stream, on a side stream with an unrelated kernel on the default stream, on a third
    stream -- the outputs cloned after each; all three equal."""
    res = []
    side, third = torch.cuda.Stream(), torch.cuda.Stream()
    big = torch.randn(1 << 24, device="cuda")
    for st in (None, side, third):
        for o in outs:
            o.fill_(float("nan")) if o.dtype.is_floating_point else o.zero_()
        torch.cuda.synchronize()
        if st is None:
            fn()
        else:
            with torch.cuda.stream(st):
                fn()
            big.mul_(1.0001)                     # unrelated work on the default stream beside it
        torch.cuda.synchronize()
        res.append([o.clone() for o in outs])
    for r in res[1:]:
        for a, b in zip(res[0], r):
            assert torch.equal(a, b)
    return res[0]


def _s():
    return torch.cuda.current_stream().cuda_stream


def test_det_sumsq_and_ordered_sum():
    L = _lib.lib()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(3_000_003, generator=g).cuda()
    out = torch.zeros(1, device="cuda")
    ws = torch.empty(256, device="cuda")

    def call():
        out.zero_()
        _lib.check(L.ast_sumsq_det(x.data_ptr(), x.numel(), out.data_ptr(), ws.data_ptr(), 256, _s()), "ast_sumsq_det")
    (r,) = _three_calls(call, [out])
    ref = float((x.double() ** 2).sum())
    assert math.isclose(float(r), ref, rel_tol=1e-5)
    parts = torch.randn(3, 7, 33, generator=g).cuda()
    o = torch.empty(3, 33, device="cuda")
    (r,) = _three_calls(lambda: _lib.check(L.ast_ordered_sum(parts.data_ptr(), 33, 7, 3, o.data_ptr(), 0, _s()), "ast_ordered_sum"), [o])
    ref = torch.zeros(3, 33, dtype=torch.float32)
    for s in range(7):
        ref += parts[:, s].cpu()
    assert torch.equal(r.cpu(), ref)                    # ascending slot order, exactly


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rows,C,Creal", [(100_000, 16, 12), (4097, 72, 72), (300, 256, 200)])
def test_det_colsum(rows, C, Creal, dtype):
    L = _lib.lib()
    x = torch.randn(rows, C, generator=torch.Generator().manual_seed(2)).to(dtype).cuda()
    out = torch.empty(Creal, device="cuda")
    ns = ops.det_slots(rows)
    ws = torch.empty(ns * Creal, device="cuda")
    base = torch.randn(Creal, generator=torch.Generator().manual_seed(3)).cuda()

    def call():
        out.copy_(base)
        _lib.check(L.ast_colsum_acc_det(x.data_ptr(), rows, C, Creal, out.data_ptr(), _lib.dcode(dtype), ws.data_ptr(), ns, _s()),
                   "ast_colsum_acc_det")
    (r,) = _three_calls(call, [out])
    ref = base.double() + x.double()[:, :Creal].sum(0)
    assert torch.allclose(r.double(), ref, rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N,HW,C", [(4, 5000, 16), (2, 777, 64), (3, 130, 512)])
def test_det_chan_stats_and_bwd_sums(N, HW, C, dtype):
    L = _lib.lib()
    g = torch.Generator().manual_seed(4)
    x = torch.randn(N, HW, C, generator=g).to(dtype).cuda()
    dy = torch.randn(N, HW, C, generator=g).to(dtype).cuda()
    r = torch.randn(N, HW, C, generator=g).to(dtype).cuda()
    sc, sh = torch.randn(C, generator=g).cuda(), torch.randn(C, generator=g).cuda()
    sc2, sh2 = torch.randn(N, C, generator=g).cuda(), torch.randn(N, C, generator=g).cuda()
    ns = ops.det_slots(HW, N)
    ws = torch.empty(N * ns * C * 3, device="cuda")
    sums = torch.empty(N, C, 2, device="cuda")
    sums3 = torch.empty(N, C, 3, device="cuda")
    dc = _lib.dcode(dtype)
    (s2,) = _three_calls(lambda: _lib.check(L.ast_chan_stats_det(x.data_ptr(), sums.data_ptr(), N, HW, C, dc, ws.data_ptr(), ns, _s()),
                                            "ast_chan_stats_det"), [sums])
    xd = x.double()
    ref = torch.stack([xd.sum(1), (xd * xd).sum(1)], -1)
    assert torch.allclose(s2.double(), ref, rtol=1e-4, atol=1e-2)

    def bwd():
        _lib.check(L.ast_norm_bwd_sums_det(dy.data_ptr(), None, x.data_ptr(), r.data_ptr(), sums3.data_ptr(), N, HW, C, 1, dc,
                                           sc.data_ptr(), sh.data_ptr(), sc2.data_ptr(), sh2.data_ptr(), ws.data_ptr(), ns, _s()),
                   "ast_norm_bwd_sums_det")
    (s3,) = _three_calls(bwd, [sums3])
    pre = xd * sc.double() + sh.double() + r.double() * sc2.double()[:, None] + sh2.double()[:, None]
    dz = dy.double() * (pre.float().double() > 0)
    ref3 = torch.stack([dz.sum(1), (dz * xd).sum(1), (dz * r.double()).sum(1)], -1)
    assert torch.allclose(s3.double(), ref3, rtol=1e-3, atol=5e-2)


@pytest.mark.parametrize("rows,D", [(12, 256), (64, 256), (7, 100)])
def test_det_layernorm_backward(rows, D):
    L = _lib.lib()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(rows, D, generator=g).cuda()
    dy = torch.randn(rows, D, generator=g).cuda()
    gamma, beta = torch.randn(D, generator=g).cuda(), torch.randn(D, generator=g).cuda()
    mean = x.mean(1)
    rstd = torch.rsqrt(x.var(1, unbiased=False) + 1e-5)
    dx, dg, db = torch.empty_like(x), torch.empty(D, device="cuda"), torch.empty(D, device="cuda")
    dsub = torch.empty_like(x)
    ws = torch.empty(2 * rows * D, device="cuda")
    g0, b0 = torch.randn(D, generator=g).cuda(), torch.randn(D, generator=g).cuda()

    def ln():
        dg.copy_(g0); db.copy_(b0)
        _lib.check(L.ast_layernorm_bwd_det(dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(),
                                           dg.data_ptr(), db.data_ptr(), rows, D, 0, ws.data_ptr(), _s()), "ast_layernorm_bwd_det")
    rdx, rdg, rdb = _three_calls(ln, [dx, dg, db])
    xh = (x.double() - mean.double()[:, None]) * rstd.double()[:, None]
    assert torch.allclose(rdg.double(), g0.double() + (dy.double() * xh).sum(0), rtol=1e-4, atol=1e-4)
    assert torch.allclose(rdb.double(), b0.double() + dy.double().sum(0), rtol=1e-4, atol=1e-4)

    def adl():
        dg.copy_(g0); db.copy_(b0)
        _lib.check(L.ast_add_drop_ln_bwd_det(dy.data_ptr(), None, x.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), None,
                                             dx.data_ptr(), dsub.data_ptr(), dg.data_ptr(), db.data_ptr(), rows, D, ws.data_ptr(), _s()),
                   "ast_add_drop_ln_bwd_det")
    adx, adg, adb = _three_calls(adl, [dx, dg, db])
    assert torch.equal(adg, rdg) and torch.equal(adb, rdb)
    assert torch.allclose(adx, rdx, rtol=1e-5, atol=1e-5)


def test_det_recon_loss_matches_default():
    L = _lib.lib()
    B, S, T, Fq = 2, 2, 287, 513
    g = torch.Generator().manual_seed(6)
    out = torch.randn(B, S, 2, T, Fq, generator=g).cuda()
    xt = torch.randn(B, S, 2, T, 597, generator=g).cuda()
    tgt = xt[..., :Fq]
    c5 = (ctypes.c_float * 5)(1.0, 0.5, 0.1, 0.2, 0.3)
    i5 = (ctypes.c_float * 5)(*([1.0 / (B * S * 2 * T * Fq)] * 5))
    n = 5 * ((B * T * Fq + 255) // 256)
    ws = torch.empty(n, device="cuda")
    res, grad = torch.empty(11, device="cuda"), torch.empty_like(out)
    rr, rg = _three_calls(lambda: _lib.check(L.ast_recon_loss_total_det(out.data_ptr(), tgt.data_ptr(), 597, B, S, T, Fq, c5, i5, ws.data_ptr(),
                                                                         n, res.data_ptr(), grad.data_ptr(), _s()), "ast_recon_loss_total_det"),
                          [res, grad])
    ws0, res0, grad0 = torch.empty(320, device="cuda"), torch.empty(11, device="cuda"), torch.empty_like(out)
    _lib.check(L.ast_recon_loss_total(out.data_ptr(), tgt.data_ptr(), 597, B, S, T, Fq, c5, i5, ws0.data_ptr(), res0.data_ptr(),
                                      grad0.data_ptr(), _s()), "ast_recon_loss_total")
    torch.cuda.synchronize()
    assert torch.equal(rg, grad0)                       # the gradient is element-wise: identical
    assert torch.allclose(rr, res0, rtol=1e-5)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_det_igemm_split_k(dtype, monkeypatch):
    """A deep, small-M layer with a plan that splits K (forced through the AST_IGEMM_FORCE tuning aid: 64 x 64 tiles, 3 K slices):
    the per-slice slabs + ordered finish repeat bitwise and match the default (atomic) form."""
    monkeypatch.setenv("AST_IGEMM_FORCE", "64,64,8,3")
    L = _lib.lib()
    N, H, W, Cs, Cd = 2, 10, 20, 256, 512                 # stride 2: the gathered kernel, K = 9 x 256, 100 output pixels
    g, (Ho, Wo) = ops.gather_direct(N, H, W, Cs, Cd, 3, 2, 1)
    dc = _lib.dcode(dtype)
    need = int(L.ast_igemm_ws_floats_det(g, dc))
    need0 = int(L.ast_igemm_ws_floats(g, dc))
    assert need0 > 0 and need > need0
    gen = torch.Generator().manual_seed(7)
    src = torch.randn(N, H, W, Cs, generator=gen).to(dtype).cuda()
    wgt = (0.05 * torch.randn(Cd, 9, Cs, generator=gen)).to(dtype).cuda()
    dst = torch.empty(N, Ho, Wo, Cd, dtype=dtype, device="cuda")
    ws = torch.empty(need, device="cuda")
    (r,) = _three_calls(lambda: _lib.check(L.ast_igemm(src.data_ptr(), wgt.data_ptr(), None, dst.data_ptr(), g, dc, 4096, ws.data_ptr(), need,
                                                       _s()), "ast_igemm det"), [dst])
    ws0 = torch.zeros(need0, device="cuda")
    d0 = torch.empty_like(dst)
    _lib.check(L.ast_igemm(src.data_ptr(), wgt.data_ptr(), None, d0.data_ptr(), g, dc, 0, ws0.data_ptr(), need0, _s()), "ast_igemm")
    torch.cuda.synchronize()
    tol = 1e-5 if dtype == torch.float32 else 1e-2
    assert torch.allclose(r.float(), d0.float(), rtol=tol, atol=tol)


def test_det_weight_grads_flush_matches_default():
    """ast_weight_grads_flush_det on a real weight bank: bitwise repeatable across streams, equal to the atomic flush within
    f32 re-association of the spectral-norm inner product."""
    ast_amd.set_compute_dtype(torch.float32)
    from ast_amd.style_encoder import _module_bank
    enc = ast_amd.ContentEncoder().cuda().train()
    bank = _module_bank(enc)
    bank.prepare(True)
    torch.cuda.synchronize()
    for i, e in enumerate(bank.entries):                  # seeded packed gradients in every weight's staging
        if e.dwp is not None:
            e.dwp.copy_(torch.randn(e.dwp.numel(), generator=torch.Generator().manual_seed(i)).cuda())
    dwp0 = [None if e.dwp is None else e.dwp.clone() for e in bank.entries]
    grads = [p for p in enc.parameters()]
    for p in grads:
        p.grad = torch.zeros_like(p)
    bank._build(True)                                     # descriptors point at the gradients just created
    ws = torch.empty(bank.ntiles, device="cuda")
    L = _lib.lib()

    def reset():
        for e, d in zip(bank.entries, dwp0):
            e.gtmp.zero_()                                # <dWp, W/sigma>: the atomic flush adds into it (prepare zeroes it)
            if d is not None:
                e.dwp.copy_(d)
        for p in grads:
            p.grad.zero_()

    def det():
        reset()
        _lib.check(L.ast_weight_grads_flush_det(bank.d_train.data_ptr(), bank.d_tiles.data_ptr(), bank.ntiles, ws.data_ptr(), ws.numel(),
                                                _s()), "ast_weight_grads_flush_det")
    outs = _three_calls(det, [])
    g_det = [p.grad.clone() for p in grads]
    reset()
    _lib.check(L.ast_weight_grads_flush_t(bank.d_train.data_ptr(), bank.d_tiles.data_ptr(), bank.ntiles, _s()), "ast_weight_grads_flush_t")
    torch.cuda.synchronize()
    assert any(float(g.abs().max()) > 0 for g in g_det)
    for a, b in zip(g_det, grads):
        assert torch.allclose(a, b.grad, rtol=1e-4, atol=1e-6)
    det()
    torch.cuda.synchronize()
    for a, p in zip(g_det, grads):
        assert torch.equal(a, p.grad)


# ---- parity of the benchmarked configuration with the oracle, in deterministic mode ----------------------------------------------
# (test_gpu_bench_config.py's helpers; bounds = 1.5 x the values measured once on the MI355X -- DESIGN 10 -- which no longer move)
# Measured (relative loss error; whole-model gradient relative L2):
#   f32:  rec 0, nce 1.2e-7, hsic 8.1e-6, adv_d 1.3e-7, adv_g 0, total 6.1e-7; style 1.84e-3, content 2.08e-4, decoder 3.72e-4
#   bf16: rec 1.50e-4, nce 5.7e-6, hsic 3.40e-2, adv_d 5.33e-4, adv_g 1.72e-4, total 8.27e-4; style 0.250, content 0.0528, decoder 0.0422
# (loss bounds floored at 1e-6 / 1e-5: the oracle side is a CPU computation whose last bits may differ between CPU machines)
DET_BOUNDS = {
    "f32": ({"*": 1e-6, "hsic": 1.2e-5, "total": 1e-6}, {"style": 2.8e-3, "content": 3.1e-4, "decoder": 5.6e-4}),
    "bf16": ({"rec": 2.25e-4, "nce": 1e-5, "hsic": 0.051, "adv_d": 8.0e-4, "adv_g": 2.6e-4, "total": 1.24e-3},
             {"style": 0.375, "content": 0.079, "decoder": 0.063}),
}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_benchmarked_configuration_vs_oracle_deterministic(dtype):
    from test_gpu_bench_config import B, S, grad_errors, oracle_reference, seeded_trainer
    from oracle import seeded_params as sp
    tol, gtol = DET_BOUNDS[dtype]
    ref = oracle_reference(True)
    try:
        with ast_amd.deterministic():
            tr = seeded_trainer(torch.float32 if dtype == "f32" else torch.bfloat16)
            x, labels = sp.seeded_input(B, S).cuda(), sp.balanced_labels(B)
            out = {k: float(v) for k, v in tr.step(x, labels).items()}
            torch.cuda.synchronize()
        errs = grad_errors(tr, ref["grads"])
        rel = {k: abs(out[k] - ref["losses"][k]) / abs(ref["losses"][k]) for k in ("rec", "nce", "hsic", "adv_d", "adv_g", "total") if k in out}
        print(f"[bench-config parity, deterministic] {dtype}: loss rel err " + ", ".join(f"{k} {v:.3e}" for k, v in rel.items())
              + "  grad rel-L2 " + ", ".join(f"{k} {v:.4e}" for k, v in errs.items()))
        for k, v in rel.items():
            assert v <= tol.get(k, tol.get("*")), (dtype, k, v)
        for k, v in errs.items():
            assert v <= gtol[k], (dtype, k, v)
    finally:
        ast_amd.set_compute_dtype(torch.float32)
