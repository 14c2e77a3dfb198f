"""Validation without a GPU: the float64 reference of the per-clip reconstruction loss (tests/recon_len_ref.py) is held to
oracle.ast_oracle.comprehensive_loss (pinned to the real reference by tests/golden/), which makes it the yardstick of the GPU
tests; the host checks of ast_recon_loss_len and its workspace query refuse every bad call before any launch; the Python entry
points refuse bad inputs with a ValueError naming the argument."""
import ctypes

import numpy as np
import pytest
import torch

import ast_amd
from ast_amd import _lib
from oracle import ast_oracle as O

import recon_len_ref as R

FAKE = 0x10000                                   # non-null, never dereferenced: every call with it below fails validation first


def _oracle_row(out, tgt, n, mse_weight):
    r = O.comprehensive_loss(torch.from_numpy(out[:, :n]).double(), torch.from_numpy(tgt[:, :n]).double(), mse_weight=mse_weight)
    return [float(r[k]) for k in ("total_loss",) + R.KEYS]


@pytest.mark.parametrize("mse_weight", sorted(R.WEIGHTS.values()))
def test_reference_follows_the_oracle_on_every_clip_of_a_ragged_batch(mse_weight):
    B, S, T, F, ld = 4, 3, 5, 7, 9
    out, x = R.make_case(B, S, T, F, ld, seed=3)
    tgt = x[..., :F]
    n = [3, 1, 2, 7]                                                    # 7 clamps to S
    res = R.recon_len_ref(out, tgt, n, mse_weight=mse_weight)
    for b, nb in enumerate(R.clamp_sections(n, B, S)):
        ref = _oracle_row(out[b:b + 1], tgt[b:b + 1], int(nb), mse_weight)
        got = [res[b, 5]] + list(res[b, 6:])
        for g, r in zip(got, ref):
            assert abs(g - r) <= 1e-12 * abs(r), (b, g, r)
    # n_sections=None is the full batch clip by clip, and the mean of the per-clip means is the batch value (equal lengths)
    full = R.recon_len_ref(out, tgt, None, mse_weight=mse_weight)
    batch = _oracle_row(out, tgt, S, mse_weight)
    for j, r in zip([5, 6, 7, 8, 9, 10], batch):
        assert abs(full[:, j].mean() - r) <= 1e-12 * abs(r)


def test_reference_edge_cases():
    B, S, T, F, ld = 3, 3, 5, 7, 9
    out, x = R.make_case(B, S, T, F, ld, seed=4)
    tgt = x[..., :F].copy()
    n = [3, 1, 2]
    res = R.recon_len_ref(out, tgt, n)
    assert res[1, 3] == 0.0 and res[1, 9] == 0.0 and res[0, 9] > 0 and res[2, 9] > 0      # temporal term exactly 0 at n_b == 1
    # the inputs really exercise both signs of the wrap and |out| = 0
    d = np.arctan2(out[:, :, 1], out[:, :, 0]).astype(np.float64) - np.arctan2(tgt[:, :, 1], tgt[:, :, 0])
    assert (d > np.pi).any() and (d < -np.pi).any() and ((out[:, :, 0] == 0) & (out[:, :, 1] == 0)).any()
    # padded sections filled with NaN change nothing, and the last real section does not look at its successor
    on, tn = out.copy(), tgt.copy()
    for b, nb in enumerate(n):
        on[b, nb:], tn[b, nb:] = np.nan, np.nan
    assert np.array_equal(R.recon_len_ref(on, tn, n), res)
    assert R.recon_len_ref(out[:, :, :, :1], tgt[:, :, :, :1], n)[:, 10].tolist() == [0.0, 0.0, 0.0]      # T == 1: no axis-3 difference


def test_symbols_are_declared_and_loaded():
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ast_hip.h")).read()
    for name in ("ast_recon_loss_len", "ast_recon_loss_len_ws_floats"):
        assert name in _lib.EXPORTS and name in _lib._SIGS and hasattr(_lib.lib(), name) and name + "(" in header
    assert "ast_recon_loss_len" in _lib.CALL_BYTES
    assert ast_amd.reconstruction_losses is ast_amd.losses.reconstruction_losses


def _refused(rc, entry, needle):
    err = _lib.lib().ast_last_error()
    assert rc != 0 and entry in err and needle in err, (rc, err)


def test_entries_refuse_bad_arguments():
    """ast_recon_loss_len and its workspace query validate before they launch."""
    lib = _lib.lib()
    c5 = (ctypes.c_float * 5)(2.0, 0.5, 0.2, 0.3, 0.1)
    assert lib.ast_recon_loss_len_ws_floats(3, 3, 5, 7) == 5 * 3 * 1                     # 35 bins: one workgroup per clip
    assert lib.ast_recon_loss_len_ws_floats(2, 2, 287, 513) == 5 * 2 * 576
    assert lib.ast_recon_loss_len_ws_floats(1, 2, 3, 400000) == 5 * 4096                 # capped: threads stride over the bins
    need = 5 * 2 * 576
    for args in ((0, 2, 287, 513), (2, 0, 287, 513), (2, 2, 0, 513), (2, 2, 287, 0), (-1, 2, 287, 513), (65536, 1, 1, 1),
                 (16, 1, 287 * 513, 1024)):                                              # B*T*Fq = 2^31 * 1.12
        assert lib.ast_recon_loss_len_ws_floats(*args) < 0, args
        _refused(-1, b"ast_recon_loss_len_ws_floats", b"bad sizes")

    def call(**kw):
        a = dict(out=FAKE, tgt=FAKE, ld=597, B=2, S=2, T=287, Fq=513, n=FAKE, c=c5, ws=FAKE, wsn=need, res=FAKE)
        a.update(kw)
        return lib.ast_recon_loss_len(a["out"], a["tgt"], a["ld"], a["B"], a["S"], a["T"], a["Fq"], a["n"], a["c"], a["ws"], a["wsn"],
                                      a["res"], None)

    for kw, needle in ((dict(out=None), b"null"), (dict(tgt=None), b"null"), (dict(c=None), b"null"), (dict(ws=None), b"null"),
                       (dict(res=None), b"null"), (dict(B=0), b">= 1"), (dict(S=0), b">= 1"), (dict(T=0), b">= 1"), (dict(Fq=0), b">= 1"),
                       (dict(S=-2), b">= 1"), (dict(ld=512), b"tgt_ld"), (dict(B=16, T=287 * 513, Fq=1024, ld=1024), b"2^31"),
                       (dict(B=65536, T=1, Fq=1, ld=1), b"65535"), (dict(wsn=need - 1), b"ws needs")):
        _refused(call(**kw), b"ast_recon_loss_len", needle)


def test_valid_call_passes_the_checks_up_to_the_launch():
    """NULL n_sections is valid (every clip full).  Without a device the failure is the runtime's, with one the call runs on zeros."""
    lib = _lib.lib()
    c5 = (ctypes.c_float * 5)(2.0, 0.5, 0.2, 0.3, 0.1)
    if torch.cuda.is_available():
        o, ws, res = torch.zeros(2, 2, 2, 5, 7, device="cuda"), torch.zeros(10, device="cuda"), torch.zeros(2, 11, device="cuda")
        assert lib.ast_recon_loss_len(o.data_ptr(), o.data_ptr(), 7, 2, 2, 5, 7, None, c5, ws.data_ptr(), 10, res.data_ptr(), None) == 0
        torch.cuda.synchronize()
        return
    rc = lib.ast_recon_loss_len(FAKE, FAKE, 7, 2, 2, 5, 7, None, c5, FAKE, 10, FAKE, None)
    err = lib.ast_last_error()
    assert rc != 0
    for word in (b"bad args", b"null", b"2^31", b"ws needs"):
        assert word not in err, err


def test_reconstruction_losses_refuses_bad_inputs():
    ok = torch.zeros(2, 3, 2, 5, 7)
    for out, tgt, what in ((ok[0], ok, "output"), (ok.double(), ok, "output"), (ok, ok.half(), "target"), (ok, ok[:, :2], "target"),
                           (ok, ok[..., :6], "target"), (torch.zeros(2, 3, 1, 5, 7), ok, "output"), (np.zeros((2, 3, 2, 5, 7), np.float32), ok, "output"),
                           (torch.zeros(2, 0, 2, 5, 7), torch.zeros(2, 0, 2, 5, 7), "output")):
        with pytest.raises(ValueError, match=what):
            ast_amd.reconstruction_losses(out, tgt)
    for bad in (torch.zeros(2), torch.zeros(2, dtype=torch.int64), torch.zeros(3, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.int32),
                [3, 3], torch.zeros(2, dtype=torch.int32)):                               # the last one: right, but on the host
        with pytest.raises(ValueError, match="n_sections"):
            ast_amd.reconstruction_losses(ok, ok, bad)
    if not torch.cuda.is_available():
        with pytest.raises(ValueError, match="output must be on the GPU"):               # wrong device
            ast_amd.reconstruction_losses(ok, ok)
    else:
        with pytest.raises(ValueError, match="target must be on the GPU"):
            ast_amd.reconstruction_losses(ok.cuda(), ok)
        with pytest.raises(ValueError, match="mse_weight"):
            ast_amd.reconstruction_losses(ok.cuda(), ok.cuda(), mse_weight="2")


def test_teacher_forced_entry_exists_on_both_decoders_and_refuses_bad_lengths():
    from ast_amd import SimpleDecoder_TransformerOnly as SD
    from ast_amd.decoder_trunk import DecoderTrunk
    assert SD.Decoder.forward_teacher_forced is DecoderTrunk.forward_teacher_forced is ast_amd.Decoder.forward_teacher_forced
    dec = ast_amd.Decoder()
    c, k, y = torch.zeros(2, 3, 256), torch.zeros(2, 256), torch.zeros(2, 3, 2, 287, 513)
    with pytest.raises(ValueError, match="eval"):                                         # per-clip lengths do not exist in training mode
        dec.forward_teacher_forced(c, k, y, lengths=torch.zeros(2, dtype=torch.int32))
    dec.eval()
    for bad in (torch.zeros(2, dtype=torch.int64), torch.zeros(3, dtype=torch.int32), [3, 3]):
        with pytest.raises(ValueError, match="lengths"):
            dec.forward_teacher_forced(c, k, y, lengths=bad)
    with pytest.raises(ValueError, match="Expected y"):
        dec.forward_teacher_forced(c, k, y[0])


def test_evaluate_refuses_more_than_one_rank_and_unknown_decode_modes():
    """Both checks come before anything touches a device, so a bare Trainer object shows them."""
    from ast_amd import train
    tr = train.Trainer.__new__(train.Trainer)
    tr.world = 2
    with pytest.raises(ValueError, match="per process"):
        tr.evaluate(torch.zeros(2, 1, 2, 287, 597), torch.tensor([0, 1]))
    tr.world = 1
    with pytest.raises(ValueError, match="decode"):
        tr.evaluate(torch.zeros(2, 1, 2, 287, 597), torch.tensor([0, 1]), decode="greedy")
    assert train.Trainer.DECODE_MODES == ("teacher_forced", "autoregressive")
