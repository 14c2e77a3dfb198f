"""BatchNorm over the live images of a padded batch, without a GPU: the float64 formulas of tests/ragged_bn_ref.py are held to
torch.nn.BatchNorm2d under autograd on the index-selected live images (which makes them the yardstick of the GPU tests), the
compaction reference of the decoder at full lengths is oracle.ast_oracle.decoder_forward, the new entries are declared, and
new_decoder.Decoder.forward_training_ragged_bn refuses what it must while the old name still refuses everything."""
import os

import numpy as np
import pytest
import torch

import ast_amd
from ast_amd import _lib, layers, ops
from oracle import ast_oracle as O
from oracle import layout as OL

import ragged_bn_ref as R

NEW_ENTRIES = ("ast_chan_stats_len", "ast_norm_finalize_len", "ast_affine_act_len", "ast_norm_bwd_sums_len", "ast_norm_bwd_finalize_len",
               "ast_norm_bwd_apply_len", "ast_nchw_to_nhwc_len", "ast_bilinear_fwd_len", "ast_bilinear_bwd_len")


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("name", R.BN_NAMES)
def test_formulas_equal_batchnorm2d_on_the_selected_live_images(name, relu):
    B, S, H, W, C, Creal, n = R.bn_case(name)
    x, dy, gamma, beta, rm, rv = R.bn_inputs(name)
    live = R.live_mask(B, S, n)
    y, mean, var, new_rm, new_rv = R.masked_bn_relu_fwd(x, gamma, beta, rm, rv, live, relu)
    dx, dgamma, dbeta = R.masked_bn_relu_bwd(x, dy, gamma, beta, live, relu)
    bn = torch.nn.BatchNorm2d(Creal).double()
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta); bn.running_mean.copy_(rm); bn.running_var.copy_(rv)
    idx = torch.from_numpy(np.flatnonzero(live))
    xl = x.double()[idx].requires_grad_(True)
    yl = bn(xl)
    yl = torch.relu(yl) if relu else yl
    yl.backward(dy.double()[idx])
    close = lambda a, b: np.abs(np.asarray(a) - b.detach().numpy()).max() <= 1e-11 * max(1.0, float(b.detach().abs().max()))   # noqa: E731
    assert close(y[live], yl) and close(dx[live], xl.grad)
    assert not y[~live].any() and not dx[~live].any()
    assert close(dgamma, bn.weight.grad) and close(dbeta, bn.bias.grad)
    assert close(new_rm, bn.running_mean) and close(new_rv, bn.running_var)
    assert close(mean, xl.mean(dim=(0, 2, 3))) and close(var, xl.var(dim=(0, 2, 3), unbiased=False))


def test_cases_cover_what_they_claim():
    for name in R.BN_NAMES:
        B, S, H, W, C, Creal, n = R.bn_case(name)
        assert len(n) == B and C % 8 == 0 and Creal <= C
    assert R.live_mask(2, 3, (0, 9)).tolist() == [True, False, False, True, True, True]           # clamped to [1, S]
    assert R.live_mask(2, 65, (65, 1)).sum() == 66 and not R.live_mask(2, 65, (65, 1))[66:].any()   # 64 dead rows in a stretch
    assert R.live_mask(2, 3, (3, 3)).all() and R.live_mask(2, 3, None).all()
    # statistics over ALL images miss the reference by far: a kernel that forgets the mask cannot pass
    x, dy, gamma, beta, rm, rv = R.bn_inputs("one-unit")
    live = R.live_mask(3, 3, (3, 1, 2))
    y, mean, *_ = R.masked_bn_relu_fwd(x, gamma, beta, rm, rv, live)
    y_all, mean_all, *_ = R.masked_bn_relu_fwd(x, gamma, beta, rm, rv, np.ones_like(live))
    assert np.abs(mean - mean_all).max() > 0.5 and np.abs(y[live] - y_all[live]).max() > 0.1


def test_compaction_reference_at_full_lengths_is_the_oracle_decoder():
    B, S = 2, 2
    content, cls, y = R.decoder_inputs(B, S)
    content, cls, y = content.double(), cls.double(), y.double()
    with torch.no_grad():
        sd1, sd2 = (R.double_state(OL.seeded_model_state("decoder")) for _ in range(2))
        ref = O.decoder_forward(sd1, content, cls, O.Cfg(training=True, p_drop=0.0), y=y)
        got = R.compaction_decoder(sd2, content, cls, y, (S,) * B)
        assert float((got - ref).abs().max()) <= 1e-10 * float(ref.abs().max())
        for k in ("conv_encoder.1.running_var", "conv_decoder.10.running_mean", "conv_decoder.3.weight_u"):
            assert float((sd1[k] - sd2[k]).abs().max()) <= 1e-12 * max(1.0, float(sd1[k].abs().max())), k
        # a short clip: its padded sections come back as zeros and the others change (the statistics lost two images)
        short = R.compaction_decoder(R.double_state(OL.seeded_model_state("decoder")), content, cls, y, (2, 1))
        assert not short[1, 1].any() and float((short[0] - ref[0]).abs().max()) > 1e-6 * float(ref.abs().max())


def test_symbols_are_declared_and_loaded():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ast_hip.h")).read()
    for name in NEW_ENTRIES:
        assert name in _lib.EXPORTS and name in _lib._SIGS and hasattr(_lib.lib(), name) and name + "(" in header, name
    for name in ("BatchNormActLenFn", "BilinearToNCHWLenFn", "nchw_to_nhwc_len", "check_bn_len_supported"):
        assert hasattr(ops, name), name
    for name in ("bn_act_len", "conv_bn_act_len", "convT_bn_act_len"):
        assert hasattr(layers, name), name


def test_entries_refuse_bad_arguments_before_any_launch():
    lib, FAKE = _lib.lib(), 0x10000

    def refused(rc, entry, needle):
        err = lib.ast_last_error()
        assert rc != 0 and entry in err and needle in err, (rc, err)

    refused(lib.ast_chan_stats_len(FAKE, FAKE, 2, 3, 16, 8, 0, None, None), b"ast_chan_stats_len", b"n_sections")
    refused(lib.ast_chan_stats_len(FAKE, FAKE, 0, 3, 16, 8, 0, FAKE, None), b"ast_chan_stats_len", b"bad args")
    refused(lib.ast_chan_stats_len(FAKE, FAKE, 2, 3, 16, 12, 0, FAKE, None), b"ast_chan_stats_len", b"bad args")
    refused(lib.ast_chan_stats_len(FAKE, FAKE, 2, 65536, 16, 8, 0, FAKE, None), b"ast_chan_stats_len", b"65535")
    refused(lib.ast_chan_stats_len(None, FAKE, 2, 3, 16, 8, 0, FAKE, None), b"ast_chan_stats_len", b"null")
    refused(lib.ast_chan_stats_len(FAKE, FAKE, 4097, 4096, 16, 8, 0, FAKE, None), b"ast_chan_stats_len", b"2^24")      # B * S images
    refused(lib.ast_bilinear_fwd_len(FAKE, FAKE, 4097, 4096, 2, 8, 8, 4, 5, 7, 0, FAKE, None), b"ast_bilinear_fwd_len", b"2^24")
    refused(lib.ast_norm_finalize_len(FAKE, None, 2, 3, 16, 8, 9, FAKE, FAKE, FAKE, FAKE, 1e-5, FAKE, FAKE, FAKE, FAKE, FAKE, None),
            b"ast_norm_finalize_len", b"Creal")
    refused(lib.ast_affine_act_len(FAKE, FAKE, FAKE, None, 2, 3, 16, 8, 1, 0, FAKE, None), b"ast_affine_act_len", b"null")
    refused(lib.ast_norm_bwd_sums_len(FAKE, None, FAKE, FAKE, 2, 3, 16, 8, 1, 0, None, None, FAKE, None), b"ast_norm_bwd_sums_len", b"ReLU mask")
    refused(lib.ast_norm_bwd_finalize_len(FAKE, 2, 3, 16, 8, 8, FAKE, FAKE, FAKE, None, None, None, FAKE, None), b"ast_norm_bwd_finalize_len", b"null")
    refused(lib.ast_norm_bwd_apply_len(FAKE, None, FAKE, FAKE, FAKE, 2, 3, 16, 8, 1, 0, None, None, FAKE, None), b"ast_norm_bwd_apply_len", b"ReLU mask")
    refused(lib.ast_nchw_to_nhwc_len(FAKE, FAKE, 2, 3, 2, 6, 10, 120, 60, 10, 8, 0, None, None), b"ast_nchw_to_nhwc_len", b"n_sections")
    refused(lib.ast_nchw_to_nhwc_len(FAKE, FAKE, 2, 3, 9, 6, 10, 120, 60, 10, 8, 0, FAKE, None), b"ast_nchw_to_nhwc_len", b"bad args")
    refused(lib.ast_bilinear_fwd_len(FAKE, FAKE, 2, 0, 2, 8, 8, 4, 5, 7, 0, FAKE, None), b"ast_bilinear_fwd_len", b"bad args")
    refused(lib.ast_bilinear_bwd_len(FAKE, FAKE, 2, 3, 3, 8, 8, 4, 5, 7, 0, FAKE, None), b"ast_bilinear_bwd_len", b"C<=2")


def test_ops_refuse_bad_lengths_before_any_pointer_is_taken():
    bn = torch.nn.BatchNorm2d(8)
    x = torch.zeros(6, 4, 4, 8)
    n_host = torch.tensor([3, 1], dtype=torch.int32)
    for bad in (None, n_host, torch.zeros(2, dtype=torch.int64), [3, 1]):
        with pytest.raises(ValueError, match="n_sections"):
            ops.BatchNormActLenFn.apply(x, bn.weight, bn.bias, bn, True, bad, 3)
        with pytest.raises(ValueError, match="n_sections"):
            ops.BilinearToNCHWLenFn.apply(x, 2, 5, 7, bad, 3)
        with pytest.raises(ValueError, match="n_sections"):
            ops.nchw_to_nhwc_len(torch.zeros(6, 2, 6, 10), torch.float32, bad, 3)
    with pytest.raises(ValueError, match="whole number"):
        ops.BatchNormActLenFn.apply(x, bn.weight, bn.bias, bn, True, n_host, 4)
    with pytest.raises(ValueError, match="eval mode"):
        ops.BatchNormActLenFn.apply(x, bn.weight, bn.bias, bn.eval(), True, n_host, 3)
    bn.train()
    ops.set_sync_bn(1, None, force=True)
    try:
        with pytest.raises(ValueError, match="sync-BN"):
            ops.BatchNormActLenFn.apply(x, bn.weight, bn.bias, bn, True, n_host, 3)
    finally:
        ops.set_sync_bn(1)
    with ast_amd.deterministic():
        with pytest.raises(ValueError, match="deterministic mode"):
            ops.BatchNormActLenFn.apply(x, bn.weight, bn.bias, bn, True, n_host, 3)


def test_decoder_entry_point_refuses_what_it_must_and_the_old_name_still_raises():
    from ast_amd.decoder_trunk import DecoderTrunk
    c, k, y = torch.zeros(2, 3, 256), torch.zeros(2, 256), torch.zeros(2, 3, 2, 5, 7)
    n_host = torch.tensor([3, 1], dtype=torch.int32)
    dec = ast_amd.Decoder.__new__(ast_amd.Decoder)       # the refusals below come before any parameter is looked at
    torch.nn.Module.__init__(dec)
    dec.eval()
    with pytest.raises(ValueError, match="train"):                                        # eval mode
        dec.forward_training_ragged_bn(c, k, y, n_host)
    dec.train()
    for bad in (None, torch.zeros(2, dtype=torch.int64), torch.zeros(3, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.int32), [3, 1],
                n_host):                                                                   # the last one: right, but on the host
        with pytest.raises(ValueError, match="n_sections"):
            dec.forward_training_ragged_bn(c, k, y, bad)
    ops.set_sync_bn(1, None, force=True)
    try:
        with pytest.raises(ValueError, match="sync-BN"):
            dec.forward_training_ragged_bn(c, k, y, n_host)
    finally:
        ops.set_sync_bn(1)
    with ast_amd.deterministic():
        with pytest.raises(ValueError, match="deterministic mode"):
            dec.forward_training_ragged_bn(c, k, y, n_host)
    with pytest.raises(ValueError, match=r"\[B, S, 2, 287, 513\]"):
        dec.forward_training_ragged_bn(c, k, y[0], n_host)
    with pytest.raises(RuntimeError, match="1024"):                                       # 1025 token rows
        dec.forward_training_ragged_bn(torch.zeros(5, 205, 256), torch.zeros(5, 256), torch.zeros(5, 205, 2, 1, 1), torch.ones(5, dtype=torch.int32))
    # the old name keeps refusing, and names the new one
    assert ast_amd.Decoder.forward_training_ragged is DecoderTrunk.forward_training_ragged
    with pytest.raises(NotImplementedError, match="BatchNorm") as e:
        dec.forward_training_ragged(c, k, y, n_host)
    assert "forward_training_ragged_bn" in str(e.value)
