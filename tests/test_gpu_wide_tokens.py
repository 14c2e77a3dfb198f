"""Wide token path: more than 64 token rows through the ast_*_wide entry points (include/ast_hip.h), from the C ABI up to the
Trainer and StyleTransferSession.

Operators against torch float64 on the CPU at M in {65, 79, 130} (one row past the old limit, a partial 16-row tile, two 64-row
blocks plus two rows) with the bound of the <= 64-row tests of the same operators (test_gpu_ops.py: max abs error < 2e-4 of the
reference's max abs); the deterministic forms repeat bitwise across streams; BigLinearFn / LinearFn / the simple decoder / the
Trainer / StyleTransferSession at 66 token rows."""
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import ast_amd
    from ast_amd import _lib, config, layers as AL, ops, train
from oracle import seeded_params as sp

DEV = "cuda"
TOL = 2e-4                                   # test_linear_fwd_bwd / test_big_linears_of_simple_decoder / test_ffn_fused
ROWS = (65, 79, 130)
WIDE_ENTRIES = {"ast_skinny_gemm_wide", "ast_skinny_gemm_wide_ex", "ast_linear_wgrad_wide", "ast_bigk_gemm_wide_det",
                "ast_bigk_gemm_wide_det_ws_floats", "ast_bign_dgrad_wide_det", "ast_bign_dgrad_wide_det_ws_floats"}


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / max(b.abs().max().item(), 1e-12))


def _s():
    return torch.cuda.current_stream().cuda_stream


def _randn(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


# ---- operators -----------------------------------------------------------------------------------------------------------------
# One body per operator, run on the wide entries (sfx = "_wide", M in ROWS) and on the <= 64-row entries (sfx = "", M in NARROW_ROWS:
# one row, a full 16-row tile, one row past it, the third weight-gradient kernel, the limit) with the same references and bound.
NARROW_ROWS = (1, 16, 17, 33, 64)


def _skinny_gemm_case(sfx, M, N, K):
    L = _lib.lib()
    plain_fn, ex_fn = getattr(L, f"ast_skinny_gemm{sfx}"), getattr(L, f"ast_skinny_gemm{sfx}_ex")
    x, w, b = _randn(M, K, seed=1), _randn(N, K, seed=2, scale=K ** -0.5), _randn(N, seed=3)
    mm = (_randn(M, N, seed=4) > 0).float() * 1.25
    xd, wd, bd, md = x.to(DEV), w.to(DEV), b.to(DEV), mm.to(DEV)
    ref0 = x.double() @ w.double().t()
    for bias, relu in ((False, False), (True, False), (True, True)):
        y = torch.full((M, N), float("nan"), device=DEV)
        _lib.check(plain_fn(xd.data_ptr(), wd.data_ptr(), bd.data_ptr() if bias else None, y.data_ptr(), M, N, K, K, N,
                            int(relu), _s()), f"ast_skinny_gemm{sfx}")
        ref = ref0 + (b.double() if bias else 0.0)
        ref = torch.relu(ref) if relu else ref
        assert rel_err(y, ref) < TOL, (bias, relu)
    # mul_mask epilogue
    y = torch.full((M, N), float("nan"), device=DEV)
    _lib.check(ex_fn(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), M, N, K, K, N, 0, md.data_ptr(), None,
                     0.0, 0, None, _s()), f"ast_skinny_gemm{sfx}_ex")
    assert rel_err(y, (ref0 + b.double()) * mm.double()) < TOL
    # dropout epilogue: the stored mask is 0 or 1/(1-p), y = relu(pre) * mask, and it is the <= 64-row entry's mask on rows 0..63.
    # For sfx = "" that comparison is ast_skinny_gemm_ex against itself at another M: it shows the mask does not depend on the
    # tiling, it is no independent reference; the values and the keep rate below are what bound the narrow mask.
    p, seed = 0.25, 12345
    ctr = torch.tensor([7], dtype=torch.int64, device=DEV)
    plain, yd, mask = (torch.full((M, N), float("nan"), device=DEV) for _ in range(3))
    _lib.check(plain_fn(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), plain.data_ptr(), M, N, K, K, N, 1, _s()), "plain")
    _lib.check(ex_fn(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), yd.data_ptr(), M, N, K, K, N, 1, None, mask.data_ptr(), p,
                     seed, ctr.data_ptr(), _s()), f"ast_skinny_gemm{sfx}_ex")
    x64 = xd if M >= 64 else torch.cat([xd, torch.zeros(64 - M, K, device=DEV)])     # the mask depends on (row, column) alone
    y64, m64 = torch.empty((64, N), device=DEV), torch.empty((64, N), device=DEV)
    _lib.check(L.ast_skinny_gemm_ex(x64.data_ptr(), wd.data_ptr(), bd.data_ptr(), y64.data_ptr(), 64, N, K, K, N, 1, None, m64.data_ptr(), p,
                                    seed, ctr.data_ptr(), _s()), "ast_skinny_gemm_ex")
    torch.cuda.synchronize()
    keep = torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(p))
    assert bool(((mask == 0) | (mask == keep.item())).all())
    assert torch.equal(mask[:64], m64[:M])
    kept = mask[plain > 0]
    if M > 64:
        assert 0.70 < float((kept > 0).float().mean()) < 0.80
    else:                                  # few rows, few draws at keep probability 0.75: 4 sigma of their count, never under 0.05
        assert abs(float((kept > 0).float().mean()) - 0.75) < max(0.05, 4 * math.sqrt(0.75 * 0.25 / kept.numel()))
    assert bool((mask[plain <= 0] == 0).all())
    assert torch.equal(yd, plain * torch.where(plain > 0, mask, torch.zeros_like(mask)))
    assert rel_err(plain, torch.relu(ref0 + b.double())) < TOL


@pytest.mark.parametrize("N,K", [(256, 256), (1024, 256), (256, 1024), (40, 256)])
@pytest.mark.parametrize("M", ROWS)
def test_skinny_gemm_wide(M, N, K):
    _skinny_gemm_case("_wide", M, N, K)


@pytest.mark.parametrize("N,K", [(256, 256), (40, 256), (256, 1024)])
@pytest.mark.parametrize("M", NARROW_ROWS)
def test_skinny_gemm_narrow(M, N, K):
    _skinny_gemm_case("", M, N, K)


def _linear_wgrad_case(sfx, M, N, K):
    fn, name = getattr(_lib.lib(), f"ast_linear_wgrad{sfx}"), f"ast_linear_wgrad{sfx}"
    dy, x = _randn(M, N, seed=5), _randn(M, K, seed=6)
    dW0, db0 = _randn(N, K, seed=7), _randn(N, seed=8)                # non-zero: the entry accumulates
    dW, db = dW0.to(DEV), db0.to(DEV)
    dyd, xd = dy.to(DEV), x.to(DEV)

    def call():
        dW.copy_(dW0); db.copy_(db0)
        _lib.check(fn(dyd.data_ptr(), xd.data_ptr(), dW.data_ptr(), db.data_ptr(), M, N, K, N, K, _s()), name)
    from test_gpu_deterministic import _three_calls
    rW, rb = _three_calls(call, [dW, db])                              # deterministic by construction
    assert rel_err(rW, dW0.double() + dy.double().t() @ x.double()) < TOL
    assert rel_err(rb, db0.double() + dy.double().sum(0)) < TOL
    call()                                                             # db == NULL: dW only
    dW.copy_(dW0)
    _lib.check(fn(dyd.data_ptr(), xd.data_ptr(), dW.data_ptr(), None, M, N, K, N, K, _s()), name)
    torch.cuda.synchronize()
    assert torch.equal(dW, rW)


@pytest.mark.parametrize("N,K", [(256, 256), (40, 100), (2050, 256), (256, 2050)])
@pytest.mark.parametrize("M", ROWS)
def test_linear_wgrad_wide(M, N, K):
    _linear_wgrad_case("_wide", M, N, K)


@pytest.mark.parametrize("N,K", [(40, 100), (256, 256)])
@pytest.mark.parametrize("M", NARROW_ROWS)
def test_linear_wgrad_narrow(M, N, K):
    _linear_wgrad_case("", M, N, K)


def _bigk_gemm_case(sfx, M):
    from test_gpu_deterministic import _three_calls
    L = _lib.lib()
    fn, det_fn, ws_fn = (getattr(L, f"ast_bigk_gemm{sfx}{t}") for t in ("", "_det", "_det_ws_floats"))
    N, K = 256, 2050                                                   # K even, not a multiple of 4; last chunk holds 2
    x, w, b = _randn(M, K, seed=9, scale=0.1), _randn(N, K, seed=10, scale=0.05), _randn(N, seed=11, scale=0.1)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    ref = x.double() @ w.double().t() + b.double()
    y = torch.full((M, N), float("nan"), device=DEV)
    _lib.check(fn(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), M, N, K, N, _s()), f"ast_bigk_gemm{sfx}")
    assert rel_err(y, ref) < TOL
    need = int(ws_fn(M, N, K))
    assert need == 3 * M * N
    ws = torch.full((need,), float("nan"), device=DEV)
    yd = torch.empty((M, N), device=DEV)
    (r,) = _three_calls(lambda: _lib.check(det_fn(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), yd.data_ptr(), M, N, K,
                                                  ws.data_ptr(), need, _s()), f"ast_bigk_gemm{sfx}_det"), [yd])
    assert rel_err(r, ref) < TOL
    _lib.check(det_fn(xd.data_ptr(), wd.data_ptr(), None, yd.data_ptr(), M, N, K, ws.data_ptr(), need, _s()), "no bias")
    assert rel_err(yd, ref - b.double()) < TOL


@pytest.mark.parametrize("M", ROWS)
def test_bigk_gemm_wide(M):
    _bigk_gemm_case("_wide", M)


@pytest.mark.parametrize("M", NARROW_ROWS)
def test_bigk_gemm_narrow(M):
    _bigk_gemm_case("", M)


def _bign_dgrad_case(sfx, M, K):
    from test_gpu_deterministic import _three_calls
    L = _lib.lib()
    fn, det_fn, ws_fn = (getattr(L, f"ast_bign_dgrad{sfx}{t}") for t in ("", "_det", "_det_ws_floats"))
    N = 2050
    dy, w = _randn(M, N, seed=12, scale=0.1), _randn(N, K, seed=13, scale=0.05)
    dyd, wd = dy.to(DEV), w.to(DEV)
    ref = dy.double() @ w.double()
    dx = torch.full((M, K), float("nan"), device=DEV)
    _lib.check(fn(dyd.data_ptr(), wd.data_ptr(), dx.data_ptr(), M, N, K, N, _s()), f"ast_bign_dgrad{sfx}")
    assert rel_err(dx, ref) < TOL
    need = int(ws_fn(M, N, K))
    assert need == 5 * M * K
    ws = torch.full((need,), float("nan"), device=DEV)
    dxd = torch.empty((M, K), device=DEV)
    (r,) = _three_calls(lambda: _lib.check(det_fn(dyd.data_ptr(), wd.data_ptr(), dxd.data_ptr(), M, N, K, N, ws.data_ptr(),
                                                  need, _s()), f"ast_bign_dgrad{sfx}_det"), [dxd])
    assert rel_err(r, ref) < TOL


@pytest.mark.parametrize("K", [256, 100])
@pytest.mark.parametrize("M", ROWS)
def test_bign_dgrad_wide(M, K):
    _bign_dgrad_case("_wide", M, K)


@pytest.mark.parametrize("K", [256, 100])
@pytest.mark.parametrize("M", NARROW_ROWS)
def test_bign_dgrad_narrow(M, K):
    _bign_dgrad_case("", M, K)


# ---- batched weight gradients: records of distinct destinations (records that share a dW race by design) ----------------------------
def _wgrad_records(shapes, seed0):
    """[(LinWg record, dW, db or None, float64 reference of dW, of db)]; every second record has db == NULL"""
    out = []
    for j, (M, N, K) in enumerate(shapes):
        dy, x = _randn(M, N, seed=seed0 + 4 * j), _randn(M, K, seed=seed0 + 4 * j + 1)
        dW0, db0 = _randn(N, K, seed=seed0 + 4 * j + 2), _randn(N, seed=seed0 + 4 * j + 3)
        t = dict(dy=dy.to(DEV), x=x.to(DEV), dW=dW0.to(DEV), db=db0.to(DEV) if j % 2 == 0 else None)
        rec = _lib.LinWg(dy=t["dy"].data_ptr(), x=t["x"].data_ptr(), dW=t["dW"].data_ptr(), db=t["db"].data_ptr() if t["db"] is not None else None,
                         M=M, N=N, K=K, lddy=N, ldw=K, p0=0, p1=0, p2=0)
        out.append((rec, t, dW0.double() + dy.double().t() @ x.double(), db0.double() + dy.double().sum(0)))
    return out


def _check_wgrad_records(items):
    torch.cuda.synchronize()
    for j, (_, t, rW, rb) in enumerate(items):
        assert rel_err(t["dW"], rW) < TOL, j
        if t["db"] is not None:
            assert rel_err(t["db"], rb) < TOL, j


@pytest.mark.parametrize("form", ["host", "device"])
def test_linear_wgrad_batched_forms(form):
    import ctypes as C
    shapes = [(5, 40, 100), (17, 256, 256), (64, 70, 130)]
    items = _wgrad_records(shapes, seed0=100)
    assert sum(t["db"] is None for _, t, _, _ in items) == 1
    arr = (_lib.LinWg * len(items))(*[it[0] for it in items])
    max_tiles = max(((K + 63) // 64) * ((N + 63) // 64) for _, N, K in shapes)
    if form == "host":
        _lib.check(_lib.lib().ast_linear_wgrad_batched_host(C.addressof(arr), len(items), max_tiles, _s()), "ast_linear_wgrad_batched_host")
    else:
        table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
        _lib.check(_lib.lib().ast_linear_wgrad_batched(table.data_ptr(), len(items), max_tiles, _s()), "ast_linear_wgrad_batched")
    _check_wgrad_records(items)


def test_linear_wgrad_batched_host_splits_past_56_records():
    import ctypes as C
    items = _wgrad_records([(3, 16, 64)] * 57, seed0=1000)             # one more than a kernel argument holds
    arr = (_lib.LinWg * len(items))(*[it[0] for it in items])
    _lib.check(_lib.lib().ast_linear_wgrad_batched_host(C.addressof(arr), len(items), 1, _s()), "ast_linear_wgrad_batched_host")
    _check_wgrad_records(items)


# ---- autograd functions at 66 rows -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("det", [False, True], ids=["default", "deterministic"])
def test_big_linear_fn_66_rows(det):
    rows, BIG = 66, 2050
    torch.manual_seed(23)
    lin_in, lin_out = nn.Linear(BIG, 256).to(DEV), nn.Linear(256, BIG).to(DEV)
    with torch.no_grad():
        lin_in.bias.normal_(0, 0.1); lin_out.bias.normal_(0, 0.1)
    x, h = torch.randn(rows, BIG) * 0.1, torch.randn(rows, 256)
    with ast_amd.deterministic(det):
        wr, br = lin_in.weight.detach().cpu().double().requires_grad_(True), lin_in.bias.detach().cpu().double().requires_grad_(True)
        yr = F.linear(x.double(), wr, br)
        gy = torch.randn(rows, 256)
        yr.backward(gy.double())
        y = ops.BigLinearFn.apply(x.to(DEV), lin_in.weight, lin_in.bias)
        assert rel_err(y, yr) < TOL
        y.backward(gy.to(DEV))
        assert rel_err(lin_in.weight.grad, wr.grad) < TOL and rel_err(lin_in.bias.grad, br.grad) < TOL
        wr, br = lin_out.weight.detach().cpu().double().requires_grad_(True), lin_out.bias.detach().cpu().double().requires_grad_(True)
        hr = h.double().requires_grad_(True)
        yr = F.linear(hr, wr, br)
        gy = torch.randn(rows, BIG) * 0.1
        yr.backward(gy.double())
        hh = h.to(DEV).requires_grad_(True)
        y = ops.BigLinearFn.apply(hh, lin_out.weight, lin_out.bias)
        assert rel_err(y, yr) < TOL
        y.backward(gy.to(DEV))
        assert rel_err(hh.grad, hr.grad) < TOL
        assert rel_err(lin_out.weight.grad, wr.grad) < TOL and rel_err(lin_out.bias.grad, br.grad) < TOL


def test_big_linear_fn_names_the_cap():
    w, b = torch.zeros(256, 2050, device=DEV), torch.zeros(256, device=DEV)
    with pytest.raises(RuntimeError, match="1024"):
        ops.BigLinearFn.apply(torch.zeros(1025, 2050, device=DEV), w, b)


def _bank(mods):
    config.set_compute_dtype(torch.float32)
    bank = AL.WeightBank()
    return bank, [bank.add(m.weight, "linear", AL.tok_dtype, bias=m.bias) for m in mods]


@pytest.mark.parametrize("fin,fout,relu", [(256, 768, False), (1024, 256, False), (256, 1024, True)])
@pytest.mark.parametrize("det", [False, True], ids=["default", "deterministic"])
def test_linear_fn_66_rows(det, fin, fout, relu):
    rows = 66
    torch.manual_seed(2)
    m = nn.Linear(fin, fout).to(DEV)
    x = torch.randn(rows, fin)
    xr = x.double().requires_grad_(True)
    wr, br = m.weight.detach().cpu().double().requires_grad_(True), m.bias.detach().cpu().double().requires_grad_(True)
    yr = F.linear(xr, wr, br)
    yr = torch.relu(yr) if relu else yr
    gy = torch.randn(rows, fout)
    yr.backward(gy.double())
    raw = _lib.lib()
    with ast_amd.deterministic(det):
        bank, (pw,) = _bank([m])
        bank.prepare(True)
        rec = _Recorder(raw)
        _lib._lib = rec
        try:
            xh = x.to(DEV).requires_grad_(True)
            y = AL.linear(xh, pw, relu=relu)
            y.backward(gy.to(DEV))
            bank._flush()
            torch.cuda.synchronize()
        finally:
            _lib._lib = raw
    names = {n for n, _ in rec.calls}
    if det:
        assert "ast_skinny_gemm_wide" in names and "ast_igemm" not in names and "ast_wgrad" not in names, sorted(names)
        tol = TOL
    else:
        assert "ast_skinny_gemm_wide" not in names, sorted(names)       # default mode keeps its igemm path above 64 rows
        tol = TOL
    assert rel_err(y, yr) < tol
    assert rel_err(xh.grad, xr.grad) < tol
    assert rel_err(m.weight.grad, wr.grad) < tol and rel_err(m.bias.grad, br.grad) < tol


def test_linear_fn_without_bank_and_ffn_deterministic_66_rows():
    """Deterministic mode: a bank-less linear takes ast_linear_wgrad_wide; ffn() keeps its fused two-launch form on the wide _ex
    entry (mask drawn in linear1's epilogue, applied in the backward's epilogue)."""
    rows = 66
    torch.manual_seed(21)
    l1, l2 = nn.Linear(256, 1024).to(DEV), nn.Linear(1024, 256).to(DEV)
    x = torch.randn(rows, 256)
    gy = torch.randn(rows, 256)
    raw = _lib.lib()
    with ast_amd.deterministic(True):
        bank, (pw1, pw2) = _bank([l1, l2])
        bank.prepare(True)
        ops._DropState.calls = 3000
        rec = _Recorder(raw)
        _lib._lib = rec
        try:
            xh = x.to(DEV).requires_grad_(True)
            y = ops.ffn(xh, pw1, pw2, 0.25, training=True)
            mask = y.grad_fn.saved_tensors[2]                           # FFNFn saves (x, h, combined mask)
            y.backward(gy.to(DEV))
            bank._flush()
            torch.cuda.synchronize()
        finally:
            _lib._lib = raw
        names = [n for n, _ in rec.calls]
        assert names.count("ast_skinny_gemm_wide_ex") == 2 and names.count("ast_skinny_gemm_wide") == 2, names
        assert "ast_dropout_fwd" not in names and "ast_igemm" not in names
        mk = mask.cpu().double()
        xr = x.double().requires_grad_(True)
        w1, b1, w2, b2 = [t.detach().cpu().double().requires_grad_(True) for t in (l1.weight, l1.bias, l2.weight, l2.bias)]
        yr = F.linear(F.linear(xr, w1, b1) * mk, w2, b2)                # the stored mask is the combined ReLU & dropout mask
        yr.backward(gy.double())
        assert 0.3 < float((mk > 0).double().mean()) < 0.45              # ~half pass the ReLU, 3/4 of those are kept
        assert rel_err(y, yr) < TOL and rel_err(xh.grad, xr.grad) < TOL
        for got, ref in ((l1.weight.grad, w1.grad), (l1.bias.grad, b1.grad), (l2.weight.grad, w2.grad), (l2.bias.grad, b2.grad)):
            assert rel_err(got, ref) < TOL
        # no bank: the weight gradient goes straight into the parameter gradient through ast_linear_wgrad_wide
        pw1.bank, saved = None, pw1.bank
        l1.zero_grad()
        rec = _Recorder(raw)
        _lib._lib = rec
        try:
            xh = x.to(DEV).requires_grad_(True)
            y = ops.LinearFn.apply(xh, pw1.weight, pw1, False)
            g1 = torch.randn(rows, 1024)
            y.backward(g1.to(DEV))
            torch.cuda.synchronize()
        finally:
            _lib._lib = raw
            pw1.bank = saved
        assert "ast_linear_wgrad_wide" in {n for n, _ in rec.calls}
        assert rel_err(l1.weight.grad, g1.double().t() @ x.double()) < TOL and rel_err(l1.bias.grad, g1.double().sum(0)) < TOL


# ---- the simple decoder at B*S = 66 against the oracle -------------------------------------------------------------------------
B66, S66 = 22, 3
_ORACLE = {}


def _simple_oracle():
    if not _ORACLE:
        from oracle import ast_oracle as O, layout as OL
        sd = OL.seeded_model_state("simple_decoder")
        content, cls = sp.seeded_normal((B66, S66, 256), 4101), sp.seeded_normal((B66, 256), 4102)
        y = sp.seeded_input(B66, S66, seed=4103, F=513)
        out = O.simple_decoder_forward(sd, content, cls, O.Cfg(training=True, p_drop=0.0), y=y)
        rec = O.comprehensive_loss(out, y, mse_weight=1.0)
        rec["total_loss"].backward()
        with torch.no_grad():
            inf = O.simple_decoder_forward(sd, content, cls, O.Cfg(training=False, p_drop=0.0))
        _ORACLE.update(content=content, cls=cls, y=y, out_sub=out.detach()[:, :, :, ::11, ::13].clone(), out_abs=float(out.detach().abs().sum()),
                       rec={k: float(v) for k, v in rec.items()}, inf_sub=inf[:, :, :, ::11, ::13].clone(),
                       gn={k: float(v.grad.norm()) for k, v in sd.items() if getattr(v, "grad", None) is not None},
                       gw_in=sd["stft_to_embedding.weight"].grad[::17, ::9973].clone(),
                       gw_out=sd["embedding_to_stft.weight"].grad[::9973, ::17].clone(), gb_out=sd["embedding_to_stft.bias"].grad[::9973].clone())
    return _ORACLE


@pytest.mark.parametrize("det", [False, True], ids=["default", "deterministic"])
def test_simple_decoder_66_rows_vs_oracle(det):
    """Bounds of test_simple_decoder_f32_vs_golden (test_gpu_models.py)."""
    from ast_amd import SimpleDecoder_TransformerOnly as SD
    o = _simple_oracle()
    ast_amd.set_compute_dtype(torch.float32)
    m = SD.Decoder()
    m.load_state_dict(sp.seeded_state_dict(m.state_dict(), tag="simple_decoder"))
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
        if isinstance(mod, torch.nn.MultiheadAttention):
            mod.dropout = 0.0
    m = m.to(DEV).train()
    content, cls, y = o["content"].to(DEV), o["cls"].to(DEV), o["y"].to(DEV)
    with ast_amd.deterministic(det):
        out = m(content, cls, y=y)
        rec = SD.compute_comprehensive_loss(out, y)
        rec["total_loss"].backward()
        torch.cuda.synchronize()
        assert rel_err(out[:, :, :, ::11, ::13], o["out_sub"]) < 1e-3
        assert math.isclose(float(out.abs().sum()), o["out_abs"], rel_tol=1e-3)
        for k in ("total_loss", "mse_loss", "mag_loss", "phase_loss", "temporal_loss", "spectral_loss"):
            assert math.isclose(float(rec[k]), o["rec"][k], rel_tol=1e-3, abs_tol=1e-6), k
        worst = 0.0
        for k, p in m.named_parameters():
            ref = o["gn"].get(k, 0.0)
            if ref > 1e-6:
                worst = max(worst, abs(float(p.grad.norm()) - ref) / ref)
        assert worst < 3e-2, worst
        assert rel_err(m.stft_to_embedding.weight.grad[::17, ::9973], o["gw_in"]) < 5e-3
        assert rel_err(m.embedding_to_stft.weight.grad[::9973, ::17], o["gw_out"]) < 5e-3
        assert rel_err(m.embedding_to_stft.bias.grad[::9973], o["gb_out"]) < 5e-3
        m.eval()
        with torch.no_grad():
            inf = m(content, cls)
        assert rel_err(inf[:, :, :, ::11, ::13], o["inf_sub"]) < 1e-3


# ---- Trainer, deterministic, B*S = 66 --------------------------------------------------------------------------------------------
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


def _state(tr):
    return {k: v.detach().clone() for k, v in (("G.flat_p", tr.G.flat_p), ("G.m", tr.G.m), ("G.v", tr.G.v), ("D.flat_p", tr.D.flat_p),
                                               ("D.m", tr.D.m), ("D.v", tr.D.v))}


def _run66(use_graph, dtype, decoder="new", deterministic=True, steps=2, record=False):
    ast_amd.set_compute_dtype(dtype)
    raw = _lib.lib()
    rec = _Recorder(raw) if record else None
    try:
        tr = train.Trainer(train.TrainConfig(use_graph=use_graph, multi_stream=use_graph, dropout=False, deterministic=deterministic,
                                             decoder=decoder), seed=7)
        x, labels = train.synthetic_batch(B66, S66, "cuda:0", seed=3)
        assert 0 < int(labels.sum()) < B66                         # both labels present
        if record:
            _lib._lib = rec
        hist = []
        for _ in range(steps):
            out = tr.step(x, labels)
            torch.cuda.synchronize()
            hist.append(({k: v.detach().clone() for k, v in out.items()}, _state(tr)))
        del tr
        return (hist, rec.calls) if record else hist
    finally:
        _lib._lib = raw
        ast_amd.set_compute_dtype(torch.float32)
        torch.cuda.empty_cache()


def _assert_equal_hist(a, b, what):
    assert len(a) == len(b)
    for i, ((la, sa), (lb, sb)) in enumerate(zip(a, b)):
        for k in la:
            assert torch.equal(la[k], lb[k]), (what, i, k, float(la[k]), float(lb[k]))
        for k in sa:
            assert torch.equal(sa[k], sb[k]), (what, i, k, float((sa[k].double() - sb[k].double()).abs().max()))


@pytest.mark.parametrize("decoder,dtype", [("new", "f32"), ("new", "bf16"), ("simple", "f32")])
def test_deterministic_trainer_66_rows_repeats_bitwise(decoder, dtype):
    dt = torch.float32 if dtype == "f32" else torch.bfloat16
    eager = _run66(False, dt, decoder)
    _assert_equal_hist(eager, _run66(False, dt, decoder), (decoder, dtype, "eager run to run"))
    graph = _run66(True, dt, decoder)
    _assert_equal_hist(graph, _run66(True, dt, decoder), (decoder, dtype, "graph run to run"))
    _assert_equal_hist(graph, eager, (decoder, dtype, "graph against eager"))
    assert all(math.isfinite(float(v)) for l, _ in eager for v in l.values())
    assert float(eager[0][0]["total"]) != float(eager[-1][0]["total"])


def test_deterministic_trainer_66_rows_computes_the_default_step():
    """Noise model of test_default_and_deterministic_compute_the_same_step (test_gpu_trainer.py::_noise_tolerances)."""
    from test_gpu_trainer import _assert_close_hist, _noise_tolerances
    fl = lambda hist: [{k: float(v) for k, v in l.items()} for l, _ in hist]
    ref = fl(_run66(False, torch.float32, deterministic=False))
    ref2 = fl(_run66(False, torch.float32, deterministic=False))
    tols = _noise_tolerances(ref, ref2)
    det = fl(_run66(False, torch.float32))
    _assert_close_hist(det, ref, tols, "deterministic vs default at 66 rows")


@pytest.mark.parametrize("decoder", ["new", "simple"])
def test_deterministic_step_66_rows_calls_only_deterministic_forms(decoder):
    from test_gpu_deterministic import _ALLOWED
    _, calls = _run66(False, torch.float32, decoder, steps=1, record=True)
    names = {n for n, _ in calls}
    allowed = _ALLOWED | WIDE_ENTRIES                               # the wide entries: no float atomics in the forms listed above
    assert names <= allowed, sorted(names - allowed)
    assert "ast_skinny_gemm_wide" in names and "ast_skinny_gemm_wide_ex" in names
    if decoder == "simple":
        assert {"ast_bigk_gemm_wide_det", "ast_bign_dgrad_wide_det", "ast_linear_wgrad_wide"} <= names
    for n, args in calls:
        if n == "ast_igemm":
            assert args[6] & 4096 and not (args[6] & (8 | 16 | 64)), (n, args[6])


# ---- StyleTransferSession over the simple decoder ---------------------------------------------------------------------------------
def test_session_simple_decoder_66_rows():
    from ast_amd import SimpleDecoder_TransformerOnly as SD
    ast_amd.set_compute_dtype(torch.float32)
    enc, dec = ast_amd.ContentEncoder(), SD.Decoder()
    enc.load_state_dict(sp.seeded_state_dict(enc.state_dict(), tag="content"))
    dec.load_state_dict(sp.seeded_state_dict(dec.state_dict(), tag="simple_decoder"))
    enc, dec = enc.to(DEV), dec.to(DEV)
    x = sp.seeded_input(B66, S66).to(DEV)
    cls = sp.seeded_normal((B66, 256), 4102).to(DEV)
    from ast_amd import infer
    we, oe = infer.StyleTransferSession(enc, dec, use_graph=False)(x, cls)
    wg, og = infer.StyleTransferSession(enc, dec, use_graph=True)(x, cls)
    torch.cuda.synchronize()
    assert oe.shape == (B66, S66, 2, 287, 513) and bool(torch.isfinite(we).all()) and float(oe.abs().max()) > 0
    assert rel_err(og, oe) < 1e-5 and rel_err(wg, we) < 1e-5       # the bound of test_gpu_trainer.py's session test
