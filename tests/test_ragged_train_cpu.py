"""Ragged training of the simple decoder without a GPU: the float64 references of tests/ragged_train_ref.py are held to
torch.autograd on oracle.ast_oracle.comprehensive_loss clip by clip (which makes them the yardstick of the GPU tests), the seeded
inputs keep what they promise, the host checks of every new entry refuse bad calls before any launch, and the Python entry points
refuse what they must -- while everything that refused per-clip lengths in training before still does."""
import ctypes
import os

import numpy as np
import pytest
import torch

import ast_amd
from ast_amd import _lib, ops
from oracle import ast_oracle as O

import ragged_train_ref as R

FAKE = 0x10000                                   # non-null, never dereferenced: every call with it below fails validation first
NEW_ENTRIES = ("ast_recon_loss_len_grad", "ast_recon_loss_len_grad_ws_floats", "ast_bign_dgrad_len", "ast_bign_dgrad_len_det",
               "ast_bign_dgrad_len_det_ws_floats", "ast_linear_wgrad_len")


def _autograd(out, tgt, n_sections, w, mse_weight):
    """loss and gradient from the oracle, one clip at a time, in float64"""
    B, S, _, T, _ = out.shape
    o = torch.from_numpy(out).double().requires_grad_(True)
    t = torch.from_numpy(np.ascontiguousarray(tgt)).double()
    loss = 0.0
    for b, nb in enumerate(R.clamp_sections(n_sections, B, S)):
        kw = dict(mse_weight=mse_weight)
        if T == 1:                                # the oracle's mean over the empty axis-3 difference is NaN: the term has no elements
            kw["lambda_spectral"] = 0.0
        r = O.comprehensive_loss(o[b:b + 1, :nb], t[b:b + 1, :nb], **kw)
        total = r["total_loss"] if T > 1 else (mse_weight * r["mse_loss"] + 0.5 * r["mag_loss"] + 0.2 * r["phase_loss"] + 0.3 * r["temporal_loss"])
        loss = loss + float(w[b]) * total
    loss.backward()
    return float(loss.detach()), o.grad.numpy()


@pytest.mark.parametrize("name", [c[0] for c in R.LOSS_CASES])
@pytest.mark.parametrize("weighted", [False, True])
def test_reference_loss_and_gradient_follow_autograd_on_the_oracle(name, weighted):
    out, x, F, ld, n = R.loss_case(name)
    tgt = x[..., :F]
    B = out.shape[0]
    cw = R.seeded_clip_weights(B, seed=len(name)) if weighted else None
    mse_weight = 1.0 if weighted else 2.0
    loss, grad, _ = R.ragged_loss_ref(out, tgt, n, cw, mse_weight=mse_weight)
    ref_loss, ref_grad = _autograd(out, tgt, n, np.full(B, 1.0 / B) if cw is None else cw, mse_weight)
    assert abs(loss - ref_loss) <= 1e-10 * abs(ref_loss)
    assert np.abs(grad - ref_grad).max() <= 1e-10 * np.abs(ref_grad).max()
    for b, nb in enumerate(R.clamp_sections(n, B, out.shape[1])):
        assert not grad[b, nb:].any()


@pytest.mark.parametrize("name", [c[0] for c in R.LOSS_CASES])
def test_every_case_handed_to_the_gpu_tests_is_fit_for_gradients(name):
    out, x, F, ld, n = R.loss_case(name)
    min_mag, margin, above, below = R.case_properties(out, x[..., :F])
    assert min_mag >= R.MIN_MAG and margin >= R.WRAP_MARGIN and above and below, (min_mag, margin, above, below)


def test_reference_edge_cases():
    out, x, F, ld, n = R.loss_case("small-ragged")
    tgt = x[..., :F].copy()
    loss, grad, res = R.ragged_loss_ref(out, tgt, n)
    # NaN behind the real sections reaches nothing; out-of-range lengths clamp
    on, tn = out.copy(), tgt.copy()
    for b, nb in enumerate(n):
        on[b, nb:], tn[b, nb:] = np.nan, np.nan
    l2, g2, r2 = R.ragged_loss_ref(on, tn, n)
    assert l2 == loss and np.array_equal(g2, grad) and np.array_equal(r2, res)
    l3, g3, _ = R.ragged_loss_ref(out, tgt, [out.shape[1] + 7, 0, -5])
    l4, g4, _ = R.ragged_loss_ref(out, tgt, [out.shape[1], 1, 1])
    assert l3 == l4 and np.array_equal(g3, g4)
    # equal lengths with w = 1/B: the batch loss of the oracle and its gradient
    o = torch.from_numpy(out).double().requires_grad_(True)
    batch = O.comprehensive_loss(o, torch.from_numpy(tgt).double())["total_loss"]
    batch.backward()
    lf, gf, _ = R.ragged_loss_ref(out, tgt, None)
    assert abs(lf - float(batch)) <= 1e-12 * abs(float(batch)) and np.abs(gf - o.grad.numpy()).max() <= 1e-10 * np.abs(gf).max()
    # the power of the GPU test: the UNMASKED batch gradient on the padded inputs misses the ragged reference by far more than any
    # float32 bound (ten bounds of up to 1e-3 each)
    miss = np.abs(gf - grad).max() / np.abs(grad).max()
    assert miss > 1e-2, miss


def test_masked_linear_references_are_the_clips_one_by_one():
    for M, S, n in R.LINEAR_ROWS:
        dy, w, x, _, _ = R.linear_case(M, 40, 12, seed=M)
        dx = R.masked_dgrad_ref(dy, w, S, n)
        dW, db = R.masked_wgrad_ref(dy, x, S, n)
        eW, eb = np.zeros((40, 12)), np.zeros(40)
        for b, nb in enumerate(R.clamp_sections(n, M // S, S)):
            rows = slice(b * S, b * S + nb)
            assert np.allclose(dx[rows], dy[rows].astype(np.float64) @ w.astype(np.float64), rtol=1e-13, atol=1e-13)
            assert not dx[b * S + nb:(b + 1) * S].any()
            eW += dy[rows].astype(np.float64).T @ x[rows].astype(np.float64)
            eb += dy[rows].astype(np.float64).sum(axis=0)
        assert np.allclose(dW, eW, rtol=1e-12, atol=1e-12) and np.allclose(db, eb, rtol=1e-12, atol=1e-12)
        assert R.row_mask(M, S, n).sum() == R.clamp_sections(n, M // S, S).sum()


def test_symbols_are_declared_and_loaded():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ast_hip.h")).read()
    for name in NEW_ENTRIES:
        assert name in _lib.EXPORTS and name in _lib._SIGS and hasattr(_lib.lib(), name) and name + "(" in header, name
    for name in ("ast_recon_loss_len_grad", "ast_bign_dgrad_len", "ast_bign_dgrad_len_det", "ast_linear_wgrad_len"):
        assert name in _lib.CALL_BYTES
    assert ast_amd.ragged_reconstruction_loss is ast_amd.losses.ragged_reconstruction_loss
    assert hasattr(ops, "BigOutLinearLenFn") and hasattr(ops, "ReconLenGradFn")


def _refused(rc, entry, needle):
    err = _lib.lib().ast_last_error()
    assert rc != 0 and entry in err and needle in err, (rc, err, needle)


def test_loss_entry_refuses_bad_arguments():
    lib = _lib.lib()
    c5 = (ctypes.c_float * 5)(2.0, 0.5, 0.2, 0.3, 0.1)
    for args in ((3, 3, 5, 7), (2, 2, 287, 513), (1, 2, 3, 400000), (2, 2, 1, 7)):
        assert lib.ast_recon_loss_len_grad_ws_floats(*args) == lib.ast_recon_loss_len_ws_floats(*args) > 0
    assert lib.ast_recon_loss_len_grad_ws_floats(2, 2, 287, 513) == 5 * 2 * 576
    assert lib.ast_recon_loss_len_grad_ws_floats(1, 2, 3, 400000) == 5 * 4096
    for args in ((0, 2, 287, 513), (2, 0, 287, 513), (2, 2, 0, 513), (2, 2, 287, 0), (65536, 1, 1, 1), (16, 1, 287 * 513, 1024)):
        assert lib.ast_recon_loss_len_grad_ws_floats(*args) < 0, args
        _refused(-1, b"ast_recon_loss_len_grad_ws_floats", b"bad sizes")
    need = 5 * 2 * 576

    def call(**kw):
        a = dict(out=FAKE, tgt=FAKE, ld=597, B=2, S=2, T=287, Fq=513, n=FAKE, cw=FAKE, c=c5, ws=FAKE, wsn=need, res=FAKE, loss=FAKE, grad=FAKE)
        a.update(kw)
        return lib.ast_recon_loss_len_grad(a["out"], a["tgt"], a["ld"], a["B"], a["S"], a["T"], a["Fq"], a["n"], a["cw"], a["c"], a["ws"],
                                           a["wsn"], a["res"], a["loss"], a["grad"], None)

    for kw, needle in ((dict(out=None), b"null"), (dict(tgt=None), b"null"), (dict(c=None), b"null"), (dict(ws=None), b"null"),
                       (dict(res=None), b"null"), (dict(loss=None), b"null"), (dict(grad=None), b"null"),
                       (dict(B=0), b">= 1"), (dict(S=0), b">= 1"), (dict(T=0), b">= 1"), (dict(Fq=0), b">= 1"), (dict(S=-2), b">= 1"),
                       (dict(ld=512), b"tgt_ld"), (dict(B=16, T=287 * 513, Fq=1024, ld=1024), b"2^31"),
                       (dict(B=65536, T=1, Fq=1, ld=1), b"65535"), (dict(wsn=need - 1), b"ws needs")):
        _refused(call(**kw), b"ast_recon_loss_len_grad", needle)


def test_masked_linear_entries_refuse_bad_arguments():
    lib = _lib.lib()
    N, K = 294462, 256
    assert lib.ast_bign_dgrad_len_det_ws_floats(9, 2050, 256) == 5 * 9 * 256
    assert lib.ast_bign_dgrad_len_det_ws_floats(130, N, K) == 576 * 130 * 256
    assert lib.ast_bign_dgrad_len_det_ws_floats(64, 1, 1) == 64
    for args in ((0, N, K), (1025, N, K), (9, 0, K), (9, N, 0), (9, N, 257), (9, 512 * 65536 + 1, 4)):
        assert lib.ast_bign_dgrad_len_det_ws_floats(*args) == -1, args

    def dgrad(det, **kw):
        a = dict(dy=FAKE, w=FAKE, dx=FAKE, M=12, N=N, K=K, lddy=N, S=3, n=FAKE, ws=FAKE, wsn=576 * 12 * 256)
        a.update(kw)
        if det:
            return lib.ast_bign_dgrad_len_det(a["dy"], a["w"], a["dx"], a["M"], a["N"], a["K"], a["lddy"], a["S"], a["n"], a["ws"], a["wsn"], None)
        return lib.ast_bign_dgrad_len(a["dy"], a["w"], a["dx"], a["M"], a["N"], a["K"], a["lddy"], a["S"], a["n"], None)

    for det, entry in ((False, b"ast_bign_dgrad_len"), (True, b"ast_bign_dgrad_len_det")):
        for kw, needle in ((dict(dy=None), b"null"), (dict(w=None), b"null"), (dict(dx=None), b"null"), (dict(M=0), b"bad args"),
                           (dict(M=1025, S=1), b"1..1024"), (dict(S=0), b"M % S"), (dict(S=5), b"M % S"), (dict(N=0), b"bad args"),
                           (dict(K=0), b"K <= 256"), (dict(K=257), b"K <= 256"), (dict(lddy=N - 1), b"lddy"),
                           (dict(n=FAKE + 2), b"4-byte"), (dict(dy=FAKE + 1), b"4-byte")):
            _refused(dgrad(det, **kw), entry, needle)
    _refused(dgrad(True, ws=None), b"ast_bign_dgrad_len_det", b"null")
    _refused(dgrad(True, wsn=576 * 12 * 256 - 1), b"ast_bign_dgrad_len_det", b"ws needs")

    def wgrad(**kw):
        a = dict(dy=FAKE, x=FAKE, dW=FAKE, db=FAKE, M=12, N=N, K=K, lddy=N, ldw=K, S=3, n=FAKE)
        a.update(kw)
        return lib.ast_linear_wgrad_len(a["dy"], a["x"], a["dW"], a["db"], a["M"], a["N"], a["K"], a["lddy"], a["ldw"], a["S"], a["n"], None)

    for kw, needle in ((dict(dy=None), b"null"), (dict(x=None), b"null"), (dict(dW=None), b"null"), (dict(M=0), b"bad args"),
                       (dict(M=1025, S=1), b"1..1024"), (dict(S=0), b"M % S"), (dict(S=7), b"M % S"), (dict(N=0), b"bad args"),
                       (dict(K=0), b"bad args"), (dict(lddy=N - 1), b"lddy"), (dict(ldw=K - 1), b"ldw"),
                       (dict(N=64 * 65535 + 1, lddy=64 * 65535 + 1), b"too large"), (dict(db=FAKE + 2), b"4-byte")):
        _refused(wgrad(**kw), b"ast_linear_wgrad_len", needle)


def test_valid_calls_pass_the_checks_up_to_the_launch():
    """NULL n_sections / n_valid / clip_weights / db are valid.  Without a device the failure is the runtime's, not a check's."""
    if torch.cuda.is_available():
        return                                    # with a device these would launch on fake pointers; the GPU tests run them on real ones
    lib = _lib.lib()
    c5 = (ctypes.c_float * 5)(2.0, 0.5, 0.2, 0.3, 0.1)
    calls = (lambda: lib.ast_recon_loss_len_grad(FAKE, FAKE, 7, 2, 2, 5, 7, None, None, c5, FAKE, 10, FAKE, FAKE, FAKE, None),
             lambda: lib.ast_bign_dgrad_len_det(FAKE, FAKE, FAKE, 6, 40, 12, 40, 3, None, FAKE, 6 * 12, None),
             lambda: lib.ast_linear_wgrad_len(FAKE, FAKE, FAKE, None, 6, 40, 12, 40, 12, 3, None, None))
    for call in calls:
        rc, err = call(), lib.ast_last_error()
        assert rc != 0
        for word in (b"bad args", b"null", b"2^31", b"ws needs", b"4-byte", b"too large"):
            assert word not in err, err


def test_python_entry_points_refuse_what_they_must():
    from ast_amd import SimpleDecoder_TransformerOnly as SD
    from ast_amd.decoder_trunk import DecoderTrunk
    assert SD.Decoder.forward_training_ragged is DecoderTrunk.forward_training_ragged is ast_amd.Decoder.forward_training_ragged
    c, k, y = torch.zeros(2, 3, 256), torch.zeros(2, 256), torch.zeros(2, 3, 2, 5, 7)
    n_host = torch.tensor([3, 1], dtype=torch.int32)
    dec = SD.Decoder.__new__(SD.Decoder)               # the refusals below come before any parameter is looked at
    torch.nn.Module.__init__(dec)
    dec.eval()
    with pytest.raises(ValueError, match="train"):                                       # eval mode
        dec.forward_training_ragged(c, k, y, n_host)
    dec.train()
    for bad in (None, torch.zeros(2, dtype=torch.int64), torch.zeros(3, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.int32), [3, 1],
                n_host):                                                                  # the last one: right, but on the host
        with pytest.raises(ValueError, match="n_sections"):
            dec.forward_training_ragged(c, k, y, bad)
    new = ast_amd.Decoder.__new__(ast_amd.Decoder)
    torch.nn.Module.__init__(new)
    with pytest.raises(NotImplementedError, match="BatchNorm"):
        new.train().forward_training_ragged(c, k, y, n_host)
    # more than 1024 rows: before anything is allocated (a CPU tensor would be refused by the first pointer taken)
    with pytest.raises(RuntimeError, match="1024"):
        ops.BigOutLinearLenFn.apply(torch.zeros(1025, 4, requires_grad=True), torch.zeros(8, 4), None, 1, None)
    with pytest.raises(ValueError, match="whole number"):
        ops.BigOutLinearLenFn.apply(torch.zeros(10, 4, requires_grad=True), torch.zeros(8, 4), None, 3, None)
    with pytest.raises(ValueError, match="lengths"):
        ops.BigOutLinearLenFn.apply(torch.zeros(6, 4, requires_grad=True), torch.zeros(8, 4), None, 3, n_host)
    with pytest.raises(ValueError, match="huge-input"):                                  # BigLinearFn's lengths: the huge-input direction only
        ops.BigLinearFn.apply(torch.zeros(6, 4), torch.zeros(8, 4), None, 3, n_host)
    with pytest.raises(ValueError, match="lengths"):
        ops.BigLinearFn.apply(torch.zeros(6, 8), torch.zeros(4, 8), None, 3, n_host)
    # the loss: the argument checks of reconstruction_losses under its own name, plus clip_weights
    ok = torch.zeros(2, 3, 2, 5, 7)
    for out, tgt, what in ((ok[0], ok, "output"), (ok.double(), ok, "output"), (ok, ok.half(), "target"), (ok, ok[:, :2], "target"),
                           (torch.zeros(2, 3, 1, 5, 7), ok, "output"), (np.zeros((2, 3, 2, 5, 7), np.float32), ok, "output")):
        with pytest.raises(ValueError, match="ragged_reconstruction_loss: " + what):
            ast_amd.ragged_reconstruction_loss(out, tgt)
    for bad in (torch.zeros(2), torch.zeros(2, dtype=torch.int64), torch.zeros(3, dtype=torch.int32), [3, 3], n_host):
        with pytest.raises(ValueError, match="n_sections"):
            ast_amd.ragged_reconstruction_loss(ok, ok, bad)
    if not torch.cuda.is_available():
        with pytest.raises(ValueError, match="output must be on the GPU"):               # CPU tensors
            ast_amd.ragged_reconstruction_loss(ok, ok)
    else:
        with pytest.raises(ValueError, match="target must be on the GPU"):
            ast_amd.ragged_reconstruction_loss(ok.cuda(), ok)
        for bad in (torch.zeros(2), torch.zeros(3, device="cuda"), torch.zeros(2, dtype=torch.float64, device="cuda"), [0.5, 0.5]):
            with pytest.raises(ValueError, match="clip_weights"):
                ast_amd.ragged_reconstruction_loss(ok.cuda(), ok.cuda(), None, bad)
        with pytest.raises(ValueError, match="mse_weight"):
            ast_amd.ragged_reconstruction_loss(ok.cuda(), ok.cuda(), mse_weight="2")


def test_the_old_refusals_are_still_in_place():
    """Per-clip lengths stay an inference feature of every existing name; ragged training came in through new ones."""
    from ast_amd import SimpleDecoder_TransformerOnly as SD
    n = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="eval"):
        _lib.len_tensor(n, 2, "lengths", training=True)
    dec = SD.Decoder.__new__(SD.Decoder)
    torch.nn.Module.__init__(dec)
    dec.train()
    c, k, y = torch.zeros(2, 3, 256), torch.zeros(2, 256), torch.zeros(2, 3, 2, 5, 7)
    for call in (lambda: dec(c, k, y=y, lengths=n), lambda: dec.prepare_memory(c, k, lengths=n),
                 lambda: dec.forward_inference(torch.zeros(2, 6, 256), lengths=n), lambda: dec.forward_teacher_forced(c, k, y, lengths=n)):
        with pytest.raises(ValueError, match="eval"):
            call()
    with pytest.raises(RuntimeError, match="inference only"):
        ops.big_out_linear(torch.zeros(6, 4, requires_grad=True), torch.zeros(8, 4), None, 3)
