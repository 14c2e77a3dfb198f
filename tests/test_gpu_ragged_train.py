"""Ragged training of the simple decoder on the device: ast_recon_loss_len_grad (values, scalar and gradient) against the float64
reference of tests/ragged_train_ref.py; the backward of the length-masked output linear (ast_bign_dgrad_len[_det],
ast_linear_wgrad_len) against plain float64 products over the counting rows; SimpleDecoder_TransformerOnly.Decoder
.forward_training_ragged + ast_amd.ragged_reconstruction_loss against the clips run one by one through the existing unmasked path;
and one captured graph for every mix of lengths.

The gradient bound is not a constant of this file: it is 4 x the figure the EXISTING batch kernel (ast_recon_loss_total with a
gradient pointer) reaches on the equal-length version of the same case, measured in the same process, floored at 2^-24 (the new
kernel adds one reciprocal and one product per coefficient).  The gradient is element-wise (no reduction), so the figure is the
same on every run; profiles/ragged_decoder_training/grad_errors.txt records both columns as measured on an MI355X."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import ragged_train_ref as R
import test_gpu_validation as V

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import ast_amd
    from ast_amd import _lib, ops
    from ast_amd.losses import RECON_KEYS

DEV = "cuda"
TOL = 2e-4                                   # tests/test_gpu_wide_tokens.py: the token GEMMs against float64
REL, ABS = 2e-3, 2e-4                        # tests/test_gpu_trainer.py: the f32 training step against the oracle, elementwise
F32_ROUNDING = 2.0 ** -24
LOSS_NAMES = [c[0] for c in R.LOSS_CASES]


def rel_err(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / max(b.abs().max().item(), 1e-12))


def _dev_n(n):
    return None if n is None else torch.tensor(n, dtype=torch.int32, device=DEV)


# ---- ast_recon_loss_len_grad -----------------------------------------------------------------------------------------------------
def _raw(out, x, ld, n, cw=None, mse_weight=2.0):
    """ast_recon_loss_len_grad through the C ABI on device tensors -> (res (B, 11), loss (1,), grad); every output pre-filled with NaN"""
    B, S, _, T, F = out.shape
    lib = _lib.lib()
    need = int(lib.ast_recon_loss_len_grad_ws_floats(B, S, T, F))
    nan = float("nan")
    ws, res, loss = torch.full((need,), nan, device=DEV), torch.full((B, 11), nan, device=DEV), torch.full((1,), nan, device=DEV)
    grad = torch.full_like(out, nan)
    c5 = (ctypes.c_float * 5)(mse_weight, 0.5, 0.2, 0.3, 0.1)
    _lib.check(lib.ast_recon_loss_len_grad(out.data_ptr(), x.data_ptr(), ld, B, S, T, F, None if n is None else n.data_ptr(),
                                           None if cw is None else cw.data_ptr(), c5, ws.data_ptr(), need, res.data_ptr(), loss.data_ptr(),
                                           grad.data_ptr(), None), "ast_recon_loss_len_grad")
    return res, loss, grad


def _batch_kernel(out, x, ld, mse_weight=2.0):
    """the existing ast_recon_loss_total with a gradient pointer on the same tensors, every clip full -> (res11, grad)"""
    B, S, _, T, F = out.shape
    n = B * S * T * F
    c = (mse_weight / (2 * n), 0.5 / n, 0.2 / n, 0.3 / (2 * B * (S - 1) * T * F) if S > 1 else 0.0, 0.1 / (2 * B * S * (T - 1) * F) if T > 1 else 0.0)
    inv = (1.0 / (2 * n), 1.0 / n, 1.0 / n, 1.0 / (2 * B * (S - 1) * T * F) if S > 1 else 0.0, 1.0 / (2 * B * S * (T - 1) * F) if T > 1 else 0.0)
    ws, res, grad = torch.empty(64 * 5, device=DEV), torch.empty(11, device=DEV), torch.empty_like(out)
    _lib.check(_lib.lib().ast_recon_loss_total(out.data_ptr(), x.data_ptr(), ld, B, S, T, F, (ctypes.c_float * 5)(*c), (ctypes.c_float * 5)(*inv),
                                               ws.data_ptr(), res.data_ptr(), grad.data_ptr(), None), "ast_recon_loss_total")
    return res, grad


@functools.lru_cache(maxsize=None)
def _case(name):
    """(out, x on the device, F, ld, n_sections, the float64 reference gradient of the equal-length version, the gradient bound)"""
    out, x, F, ld, n = R.loss_case(name)
    o, xd = torch.from_numpy(out).to(DEV), torch.from_numpy(x).to(DEV)
    _, full_ref, _ = R.ragged_loss_ref(out, x[..., :F], None)
    _, g = _batch_kernel(o, xd, ld)
    parent = float(np.abs(g.double().cpu().numpy() - full_ref).max() / np.abs(full_ref).max())
    return out, x, o, xd, F, ld, n, parent, 4.0 * max(parent, F32_ROUNDING)


def _grad_err(g, ref):
    return float(np.abs(g.double().cpu().numpy() - ref).max() / np.abs(ref).max())


def _value_bound(name):
    """The value bound of tests/test_gpu_validation.py, taken over as it stands: 4 x max(batch kernel's measured error, 2^-24) per
    quantity.  Its PARENT_ERR figures were measured on recon_len_ref.make_case inputs of these shapes, not on the make_grad_case
    inputs used here (no zero bins, phases away from the wrap): the bound is that file's, not one derived from these inputs -- the
    values of this kernel are recon_len_kernel's sums, which that file already holds to it.  one-frame is not among its cases and
    gets, per quantity, the smallest bound of the four (mostly the 2^-24 floor x 4); its axis-3 columns are exactly 0 on both
    sides."""
    if name in V.PARENT_ERR:
        return V._bound(name)
    return np.min([V._bound(k) for k in V.PARENT_ERR], axis=0)


@pytest.mark.parametrize("weighted", [False, True], ids=["mean", "weights"])
@pytest.mark.parametrize("name", LOSS_NAMES)
def test_loss_kernel_against_float64_reference(name, weighted):
    out, x, o, xd, F, ld, n, parent, bound = _case(name)
    B, S = out.shape[:2]
    cw = R.seeded_clip_weights(B, seed=len(name)) if weighted else None
    ref_loss, ref_grad, ref_res = R.ragged_loss_ref(out, x[..., :F], n, cw)
    cwd = None if cw is None else torch.from_numpy(cw).to(DEV)
    res, loss, grad = _raw(o, xd, ld, _dev_n(n), cwd)
    got = res.double().cpu().numpy()
    vb = _value_bound(name)
    verr = np.abs(got - ref_res) / np.maximum(np.abs(ref_res), 1e-300)
    gerr = _grad_err(grad, ref_grad)
    w = np.full(B, 1.0 / B) if cw is None else cw.astype(np.float64)
    scale = float(np.sum(np.abs(w * ref_res[:, 5])))
    lerr = abs(float(loss.double()) - ref_loss) / scale
    # the scalar: B products and B - 1 additions on top of the totals' own error, each rounding once
    lbound = vb[5] + 2 * B * F32_ROUNDING
    print(f"{name} weights={weighted}: values worst {verr.max():.2e}; loss {lerr:.2e} (bound {lbound:.2e}); "
          f"gradient {gerr:.3e} (batch kernel on the equal-length version {parent:.3e}, bound {bound:.3e})")
    assert np.isfinite(got).all() and bool(torch.isfinite(grad).all())
    assert (np.abs(got - ref_res) <= vb[None, :] * np.abs(ref_res)).all(), (name, verr.max(axis=0), vb)
    assert lerr <= lbound, (lerr, lbound)
    assert gerr <= bound, (gerr, bound)
    for b, nb in enumerate(R.clamp_sections(n, B, S)):
        assert int((grad[b, nb:] != 0).sum()) == 0, b                      # rows s >= n_b: exactly 0
        if nb == 1:
            assert got[b, 3] == 0.0 and got[b, 9] == 0.0
    if out.shape[3] == 1:
        assert not got[:, 4].any() and not got[:, 10].any()
    # the public op is the same call
    oo = o.clone().requires_grad_(True)
    l2, parts = ast_amd.ragged_reconstruction_loss(oo, xd[..., :F], _dev_n(n), cwd)
    assert l2.dim() == 0 and not parts["total_loss"].requires_grad
    (3.0 * l2).backward()
    assert torch.equal(l2.detach(), loss[0]) and torch.equal(parts["total_loss"], res[:, 5])
    for i, k in enumerate(RECON_KEYS):
        assert torch.equal(parts[k], res[:, 6 + i])
    assert _grad_err(oo.grad / 3.0, ref_grad) <= bound


@pytest.mark.parametrize("name", ["small-full", "small-ragged", "real-size"])
def test_equal_lengths_give_the_batch_loss_and_its_gradient(name):
    out, x, o, xd, F, ld, n, parent, bound = _case(name)
    S = out.shape[1]
    _, full_ref, _ = R.ragged_loss_ref(out, x[..., :F], None)
    oo = o.clone().requires_grad_(True)
    batch = ast_amd.compute_comprehensive_loss(oo, xd[..., :F])["total_loss"]
    batch.backward()
    batch = batch.detach()
    _, loss, grad = _raw(o, xd, ld, None)
    _, loss_n, grad_n = _raw(o, xd, ld, _dev_n([S] * out.shape[0]))
    assert torch.equal(grad, grad_n) and torch.equal(loss, loss_n)         # NULL n_sections: every clip full
    diff = float((grad.double() - oo.grad.double()).abs().max() / np.abs(full_ref).max())
    print(f"{name}: gradient against ReconTotalFn's {diff:.3e} (bound {bound:.3e}); loss {float(loss):.8f} against {float(batch):.8f}")
    assert diff <= bound
    # two float32 kernels that each keep the value bound against the float64 reference: twice that between them
    assert abs(float(loss) - float(batch)) <= 2 * V._bound(name)[5] * abs(float(batch))


@pytest.mark.parametrize("name", ["small-ragged", "real-size"])
def test_padded_sections_lengths_out_of_range_repeats_and_clips_alone(name):
    out, x, o, xd, F, ld, n, parent, bound = _case(name)
    B, S = out.shape[:2]
    cw = torch.from_numpy(R.seeded_clip_weights(B, seed=5)).to(DEV)

    def run(fill):
        oo, xx = o.clone(), xd.clone()
        for b, nb in enumerate(n):
            oo[b, nb:], xx[b, nb:] = fill, fill
        return _raw(oo, xx, ld, _dev_n(n), cw)

    zero = run(0.0)
    for a, c in zip(run(0.0), zero):
        assert torch.equal(a, c)                                           # a second run: bit-identical
    for fill in (float("nan"), 1e30):
        for a, c in zip(run(fill), zero):
            assert torch.equal(a.view(torch.int32), c.view(torch.int32)), fill
    # a clip alone (B = 1, S = n_b, weight w_b): its rows of the batch gradient, within the bound
    _, ref_grad, _ = R.ragged_loss_ref(out, x[..., :F], n, cw.cpu().numpy())
    for b, nb in enumerate(n):
        _, _, ga = _raw(o[b:b + 1, :nb].contiguous(), xd[b:b + 1, :nb].contiguous(), ld, None, cw[b:b + 1].clone())
        d = float((ga[0].double() - zero[2][b, :nb].double()).abs().max() / np.abs(ref_grad[b]).max())
        print(f"{name} clip {b} alone against its rows: {d:.3e} (bound {bound:.3e})")
        assert d <= bound, (b, d)
        # with the clip's weight handed over explicitly the coefficients are the same floats and every bin the same arithmetic:
        # the same bits (with clip_weights NULL, 1/B would differ between the batch and the clip alone)
        assert torch.equal(ga[0], zero[2][b, :nb]), b


def test_device_lengths_out_of_range_are_clamped():
    out, x, o, xd, F, ld, n, parent, bound = _case("small-ragged")
    S = out.shape[1]
    for a, c in zip(_raw(o, xd, ld, _dev_n([S + 7, 0, -5])), _raw(o, xd, ld, _dev_n([S, 1, 1]))):
        assert torch.equal(a, c)


def test_the_unmasked_gradient_would_fail_on_the_padded_batch():
    """The power of the gradient check: the existing unmasked gradient on the padded [3, 1, 2] inputs misses by more than ten bounds."""
    out, x, o, xd, F, ld, n, parent, bound = _case("small-ragged")
    _, ref_grad, _ = R.ragged_loss_ref(out, x[..., :F], n)
    _, g = _batch_kernel(o, xd, ld)
    miss = _grad_err(g, ref_grad)
    print(f"unmasked gradient on the padded batch misses by {miss:.3e}, bound {bound:.3e}")
    assert miss > 10 * bound


# ---- ast_bign_dgrad_len[_det], ast_linear_wgrad_len --------------------------------------------------------------------------------
def _dgrad_len(dy, w, S, n, det, fill=float("nan")):
    M, N = dy.shape
    K = w.shape[1]
    lib = _lib.lib()
    dx = torch.full((M, K), fill, device=DEV)
    nv = None if n is None else n.data_ptr()
    if det:
        need = int(lib.ast_bign_dgrad_len_det_ws_floats(M, N, K))
        assert need == ((N + 511) // 512) * M * K
        ws = torch.full((need,), float("nan"), device=DEV)
        _lib.check(lib.ast_bign_dgrad_len_det(dy.data_ptr(), w.data_ptr(), dx.data_ptr(), M, N, K, N, S, nv, ws.data_ptr(), need, None), "ast_bign_dgrad_len_det")
    else:
        _lib.check(lib.ast_bign_dgrad_len(dy.data_ptr(), w.data_ptr(), dx.data_ptr(), M, N, K, N, S, nv, None), "ast_bign_dgrad_len")
    return dx


def _dgrad_plain(dy, w, det):
    M, N = dy.shape
    K = w.shape[1]
    lib = _lib.lib()
    wide = "_wide" if M > 64 else ""
    dx = torch.full((M, K), float("nan"), device=DEV)
    if det:
        need = int(getattr(lib, f"ast_bign_dgrad{wide}_det_ws_floats")(M, N, K))
        ws = torch.empty(need, device=DEV)
        _lib.check(getattr(lib, f"ast_bign_dgrad{wide}_det")(dy.data_ptr(), w.data_ptr(), dx.data_ptr(), M, N, K, N, ws.data_ptr(), need, None), "dgrad_det")
    else:
        _lib.check(getattr(lib, f"ast_bign_dgrad{wide}")(dy.data_ptr(), w.data_ptr(), dx.data_ptr(), M, N, K, N, None), "dgrad")
    return dx


def _poison(t, M, S, n):
    """NaN in every row that does not count"""
    keep = torch.from_numpy(R.row_mask(M, S, n)).to(DEV)
    t = t.clone()
    t[~keep] = float("nan")
    return t


@pytest.mark.parametrize("K", R.LINEAR_KS)
@pytest.mark.parametrize("M,S,n", R.LINEAR_ROWS, ids=[f"M{m}" + ("" if n else "full") for m, _, n in R.LINEAR_ROWS])
def test_masked_dgrad(M, S, n, K):
    N = R.LINEAR_N
    dy_h, w_h, _, _, _ = R.linear_case(M, N, K, seed=M + K)
    dy, w = torch.from_numpy(dy_h).to(DEV), torch.from_numpy(w_h).to(DEV)
    ref = torch.from_numpy(R.masked_dgrad_ref(dy_h, w_h, S, n))
    dead = torch.from_numpy(~R.row_mask(M, S, n)).to(DEV)
    dn = _dev_n(n)
    det = _dgrad_len(dy, w, S, dn, True)
    atom = _dgrad_len(dy, w, S, dn, False)
    print(f"dgrad M={M} K={K}: deterministic {rel_err(det, ref):.2e}, atomic {rel_err(atom, ref):.2e}")
    assert rel_err(det, ref) < TOL and rel_err(atom, ref) < TOL
    for dx in (det, atom):
        assert int((dx[dead] != 0).sum()) == 0                             # rows that do not count: exactly 0 (dx arrived as NaN)
    for _ in range(2):                                                       # three calls of the deterministic form: the same bits
        assert torch.equal(_dgrad_len(dy, w, S, dn, True), det)
    if n is not None:
        assert torch.equal(_dgrad_len(_poison(dy, M, S, n), w, S, dn, True), det)     # NaN in every non-counting row of dy
        assert rel_err(_dgrad_len(_poison(dy, M, S, n), w, S, dn, False), ref) < TOL
    else:                                                                    # no mask: the existing entries
        assert torch.equal(det, _dgrad_plain(dy, w, True))
        assert rel_err(atom, _dgrad_plain(dy, w, False)) < TOL
    if n is None and M > 64:                                                 # and the one-tile form on 9 rows
        assert torch.equal(_dgrad_len(dy[:9].contiguous(), w, 3, None, True), _dgrad_plain(dy[:9].contiguous(), w, True))


def _wgrad_len(dy, x, dW0, db0, S, n):
    M, N = dy.shape
    K = x.shape[1]
    dW, db = dW0.clone(), db0.clone()
    _lib.check(_lib.lib().ast_linear_wgrad_len(dy.data_ptr(), x.data_ptr(), dW.data_ptr(), db.data_ptr(), M, N, K, N, K, S,
                                               None if n is None else n.data_ptr(), None), "ast_linear_wgrad_len")
    return dW, db


@pytest.mark.parametrize("N,K", [(R.LINEAR_N, 256), (R.LINEAR_N, 100), (100, R.LINEAR_N)], ids=["K256", "K100", "transposed"])
@pytest.mark.parametrize("M,S,n", R.LINEAR_ROWS, ids=[f"M{m}" + ("" if n else "full") for m, _, n in R.LINEAR_ROWS])
def test_masked_wgrad(M, S, n, N, K):
    dy_h, _, x_h, dW0_h, db0_h = R.linear_case(M, N, K, seed=M + K + 1)
    dy, x, dW0, db0 = (torch.from_numpy(a).to(DEV) for a in (dy_h, x_h, dW0_h, db0_h))
    rW, rb = R.masked_wgrad_ref(dy_h, x_h, S, n)
    rW, rb = torch.from_numpy(rW + dW0_h.astype(np.float64)), torch.from_numpy(rb + db0_h.astype(np.float64))
    dn = _dev_n(n)
    dW, db = _wgrad_len(dy, x, dW0, db0, S, dn)
    print(f"wgrad M={M} N={N} K={K}: dW {rel_err(dW, rW):.2e}, db {rel_err(db, rb):.2e}")
    assert rel_err(dW, rW) < TOL and rel_err(db, rb) < TOL
    dW2, db2 = _wgrad_len(dy, x, dW0, db0, S, dn)
    assert torch.equal(dW, dW2) and torch.equal(db, db2)
    if n is not None:                                                        # NaN in every non-counting row of dy and x
        dW3, db3 = _wgrad_len(_poison(dy, M, S, n), _poison(x, M, S, n), dW0, db0, S, dn)
        assert torch.equal(dW, dW3) and torch.equal(db, db3)
    else:                                                                    # no mask: the bits of the existing entries
        for rows, s in ((M, S), (9, 3)):
            a, b = _wgrad_len(dy[:rows].contiguous(), x[:rows].contiguous(), dW0, db0, s, None)
            eW, eb = dW0.clone(), db0.clone()
            name = "ast_linear_wgrad_wide" if rows > 64 else "ast_linear_wgrad"
            _lib.check(getattr(_lib.lib(), name)(dy[:rows].contiguous().data_ptr(), x[:rows].contiguous().data_ptr(), eW.data_ptr(), eb.data_ptr(),
                                                rows, N, K, N, K, None), name)
            assert torch.equal(a, eW) and torch.equal(b, eb), rows


def test_masked_linear_function_against_the_unmasked_one():
    """ops.BigOutLinearLenFn: counting rows have BigLinearFn's bits; the backward goes through the masked entries."""
    M, S, n, N, K = 9, 3, (3, 1, 2), 2050, 256
    dy_h, w_h, x_h, _, b_h = R.linear_case(M, N, K, seed=77)
    w = torch.from_numpy(w_h).to(DEV).requires_grad_(True)
    bias = torch.from_numpy(b_h).to(DEV).requires_grad_(True)
    x = torch.from_numpy(x_h).to(DEV).requires_grad_(True)
    dy = torch.from_numpy(dy_h).to(DEV)
    keep = torch.from_numpy(R.row_mask(M, S, n)).to(DEV)
    y = ops.BigOutLinearLenFn.apply(x, w, bias, S, _dev_n(n))
    plain = ops.BigLinearFn.apply(x.detach(), w.detach(), bias.detach())
    assert torch.equal(y[keep], plain[keep]) and int((y[~keep] != 0).sum()) == 0
    y.backward(_poison(dy, M, S, n))
    rW, rb = R.masked_wgrad_ref(dy_h, x_h, S, n)
    assert rel_err(w.grad, torch.from_numpy(rW)) < TOL and rel_err(bias.grad, torch.from_numpy(rb)) < TOL
    assert rel_err(x.grad, torch.from_numpy(R.masked_dgrad_ref(dy_h, w_h, S, n))) < TOL
    assert int((x.grad[~keep] != 0).sum()) == 0


# ---- the simple decoder, end to end ------------------------------------------------------------------------------------------------
def _close(got, ref, what):
    got, ref = got.detach().double(), ref.detach().double()
    bound = torch.clamp(REL * torch.maximum(got.abs(), ref.abs()), min=ABS)
    worst = float(((got - ref).abs() - bound).max())
    assert worst <= 0.0, (what, float((got - ref).abs().max()), float(ref.abs().max()))


def _set_dropout(m, p):
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = p
        if isinstance(mod, torch.nn.MultiheadAttention):
            mod.dropout = p


@pytest.fixture(scope="module")
def simple():
    """SimpleDecoder_TransformerOnly.Decoder on the suite's seeded non-zero weights (a fresh one outputs exactly 0), f32, dropout 0."""
    from ast_amd import SimpleDecoder_TransformerOnly as SD
    from oracle import seeded_params as sp
    ast_amd.set_compute_dtype(torch.float32)
    m = SD.Decoder()
    m.load_state_dict(sp.seeded_state_dict(m.state_dict(), tag="simple_decoder"))
    _set_dropout(m, 0.0)
    yield m.to(DEV).train()
    _set_dropout(m, 0.0)


def _inputs(S, n, pad):
    """content (B, S, 256), class (B, 256), y (B, S, 2, 287, 513): seeded; the padded sections of y hold `pad`, the padded rows of
    content stay finite random numbers"""
    B = len(n)
    g = torch.Generator().manual_seed(900 + S)
    content, cls = torch.randn(B, S, 256, generator=g), torch.randn(B, 256, generator=g)
    y = 0.5 * torch.randn(B, S, 2, 287, 513, generator=g)
    for b, nb in enumerate(n):
        y[b, nb:] = pad
    return content.to(DEV), cls.to(DEV), y.to(DEV)


def _ragged_step(dec, content, cls, y, n):
    for p in dec.parameters():
        p.grad = None
    c, k = content.clone().requires_grad_(True), cls.clone().requires_grad_(True)
    out = dec.forward_training_ragged(c, k, y, _dev_n(n))
    loss, parts = ast_amd.ragged_reconstruction_loss(out, y, _dev_n(n), mse_weight=1.0)
    loss.backward()
    torch.cuda.synchronize()
    return out.detach(), loss.detach(), parts, c.grad, k.grad, [p.grad.detach().clone() for p in dec.parameters()]


@pytest.mark.parametrize("S,n", [(3, [3, 1, 2]), (9, [9, 1, 2])], ids=["S3", "S9-long-attention"])
def test_decoder_on_a_padded_batch_equals_the_clips_one_by_one(simple, S, n):
    from ast_amd import SimpleDecoder_TransformerOnly as SD
    dec, B = simple, len(n)
    content, cls, y = _inputs(S, n, pad=7.5)
    out, loss, parts, dc, dk, grads = _ragged_step(dec, content, cls, y, n)
    # the clips alone through the existing unmasked path, gradients accumulating over the clips
    for p in dec.parameters():
        p.grad = None
    ref_loss = 0.0
    for b, nb in enumerate(n):
        c, k = content[b:b + 1, :nb].clone().requires_grad_(True), cls[b:b + 1].clone().requires_grad_(True)
        yb = y[b:b + 1, :nb].clone(memory_format=torch.contiguous_format)      # fresh strides: size-1 dimensions keep the batch's otherwise
        ob = dec(c, k, y=yb)
        lb = SD.compute_comprehensive_loss(ob, yb)["total_loss"] / B
        lb.backward()
        ref_loss += float(lb.detach())
        assert float(out[b, :nb].abs().min()) > 0                          # the phase gradient is defined on every real bin
        _close(out[b, :nb], ob[0], f"output of clip {b}")
        assert int((out[b, nb:] != 0).sum()) == 0, b                        # padded sections: exactly 0
        _close(dc[b, :nb], c.grad[0], f"content gradient of clip {b}")
        assert int((dc[b, nb:] != 0).sum()) == 0, b
        _close(dk[b], k.grad[0], f"class gradient of clip {b}")
        _close(parts["total_loss"][b], B * lb.detach(), f"loss of clip {b}")
    torch.cuda.synchronize()
    assert abs(float(loss) - ref_loss) <= max(REL * abs(ref_loss), ABS), (float(loss), ref_loss)
    for (name, p), g in zip(dec.named_parameters(), grads):
        _close(g, p.grad, f"gradient of {name}")


def test_decoder_deterministic_dropout_repeats_and_padded_targets_reach_nothing(simple):
    dec, S, n = simple, 3, [3, 1, 2]
    content, cls, y = _inputs(S, n, pad=0.0)
    _, _, y_nan = _inputs(S, n, pad=float("nan"))
    with ast_amd.deterministic():
        _set_dropout(dec, 0.1)
        runs = []
        for _ in range(2):
            ops._DropState.calls = 9000
            runs.append(_ragged_step(dec, content, cls, y, n))
        ops._DropState.calls = 9100
        other = _ragged_step(dec, content, cls, y, n)
        _set_dropout(dec, 0.0)
        clean = _ragged_step(dec, content, cls, y, n)
        poisoned = _ragged_step(dec, content, cls, y_nan, n)
    for a, c in ((runs[0], runs[1]), (clean, poisoned)):
        assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1]) and torch.equal(a[3], c[3]) and torch.equal(a[4], c[4])
        for g1, g2 in zip(a[5], c[5]):
            assert torch.equal(g1, g2)
    assert not torch.equal(runs[0][0], other[0])                          # the dropout is on
    assert bool(torch.isfinite(poisoned[1])) and all(bool(torch.isfinite(g).all()) for g in poisoned[5])


# ---- one captured graph for every mix of lengths -----------------------------------------------------------------------------------
def test_one_captured_graph_serves_every_mix_of_lengths():
    """BigOutLinearLenFn + ragged_reconstruction_loss, forward and backward, in a torch.cuda.graph (single stream, no parallel branch):
    replays with two contents of the lengths tensor equal their eager runs bit for bit."""
    M, S, K, T, F = 9, 3, 16, 5, 7
    N = 2 * T * F
    out_h, x_h, _, _, _ = R.loss_case("small-ragged")
    g = torch.Generator().manual_seed(123)
    h = torch.randn(M, K, generator=g).to(DEV).requires_grad_(True)
    w = (torch.randn(N, K, generator=g) * 0.5).to(DEV).requires_grad_(True)
    bias = torch.randn(N, generator=g).to(DEV).requires_grad_(True)
    tgt = torch.from_numpy(x_h).to(DEV)[..., :F]
    lengths = _dev_n([3, 1, 2])
    with ast_amd.deterministic():
        def step():
            h.grad = None
            w.grad.zero_()
            bias.grad.zero_()
            out = ops.BigOutLinearLenFn.apply(h, w, bias, S, lengths).view(3, S, 2, T, F)
            loss, parts = ast_amd.ragged_reconstruction_loss(out, tgt, lengths)
            loss.backward()
            return loss.detach(), parts["total_loss"], h.grad, w.grad, bias.grad

        w.grad, bias.grad = torch.zeros_like(w), torch.zeros_like(bias)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = step()
        seen = []
        for mix in ([3, 1, 2], [2, 3, 1]):
            lengths.copy_(_dev_n(mix))
            graph.replay()
            torch.cuda.synchronize()
            replayed = [t.clone() for t in captured]
            eager = [t.clone() for t in step()]
            torch.cuda.synchronize()
            for a, c in zip(replayed, eager):
                assert torch.equal(a, c), mix
            seen.append(replayed[0])
    assert not torch.equal(seen[0], seen[1])                              # the replay read the new lengths
