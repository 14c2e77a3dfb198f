"""The two decoders on their shared trunk (ast_amd/decoder_trunk.py), without a GPU: parameter and state_dict names in registration
order (what checkpoints, _init_weights and the seeded test parameters go by), the trunk's methods being one function object on both
classes, the order of the lengths check and the weight preparation, and the one check of a per-clip count tensor at every site that
takes one."""
import functools
import os

import numpy as np
import pytest
import torch

from ast_amd import SimpleDecoder_TransformerOnly as simple
from ast_amd import _lib, cqt, decoder_trunk, new_decoder, ops
from ast_amd import utilityFunctions as U
from ast_amd.infer import StyleTransferSession
from oracle import layout as OL

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def decoder_of(mod):
    """One instance per class for the whole file (the simple decoder's two 301 MB linears take seconds to initialise); a test
    that changes its mode or patches it puts it back."""
    return mod.Decoder().eval()


# ---- names, in registration order --------------------------------------------------------------------------------------------------
LAYER = ["self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
         "multihead_attn.in_proj_weight", "multihead_attn.in_proj_bias", "multihead_attn.out_proj.weight", "multihead_attn.out_proj.bias",
         "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias",
         "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias", "norm3.weight", "norm3.bias"]
TRUNK_PARAMS = (["content_proj.weight", "content_proj.bias", "class_proj.weight", "class_proj.bias"]
                + [f"transformer_decoder.layers.{i}.{n}" for i in range(4) for n in LAYER]
                + ["input_norm.weight", "input_norm.bias", "output_norm.weight", "output_norm.bias"])
TRUNK_STATE = (["content_proj.weight", "content_proj.bias", "class_proj.weight", "class_proj.bias", "pos_encoding.pe"]
               + [f"transformer_decoder.layers.{i}.{n}" for i in range(4) for n in LAYER]
               + ["input_norm.weight", "input_norm.bias", "output_norm.weight", "output_norm.bias"])


def _sn(p, state):                      # a spectral-normed conv: parameters bias, weight_orig; buffers weight_u, weight_v
    return [p + ".bias", p + ".weight_orig"] + ([p + ".weight_u", p + ".weight_v"] if state else [])


def _bn(p, state):
    return [p + ".weight", p + ".bias"] + ([p + ".running_mean", p + ".running_var", p + ".num_batches_tracked"] if state else [])


def _cnn_names(state):
    names = []
    for seq, slots in (("conv_encoder", (0, 3, 6, 9)), ("spatial_projection", (0,))):
        for i in slots:
            names += _sn(f"{seq}.{i}", state) + _bn(f"{seq}.{i + 1}", state)
    names += _sn("spatial_projection.3", state)
    names += ["feature_to_sequence.weight", "feature_to_sequence.bias", "sequence_to_feature.weight", "sequence_to_feature.bias"]
    for i in (0, 3, 6, 9):
        names += _sn(f"conv_decoder.{i}", state) + _bn(f"conv_decoder.{i + 1}", state)
    return names + _sn("conv_decoder.12", state)


BIG = ["stft_to_embedding.weight", "stft_to_embedding.bias", "embedding_to_stft.weight", "embedding_to_stft.bias"]
EXPECTED = {new_decoder: (["start_token"] + _cnn_names(False) + TRUNK_PARAMS, ["start_token"] + _cnn_names(True) + TRUNK_STATE),
            simple: (["start_token"] + BIG + TRUNK_PARAMS, ["start_token"] + BIG + TRUNK_STATE)}


@pytest.mark.parametrize("mod", [new_decoder, simple], ids=["new_decoder", "simple"])
def test_names_in_registration_order(mod):
    dec = decoder_of(mod)
    params, state = EXPECTED[mod]
    assert (len(params), len(state)) == ((125, 175) if mod is new_decoder else (85, 86))
    assert [n for n, _ in dec.named_parameters()] == params
    assert list(dec.state_dict().keys()) == state
    # the same lists as the oracle's layout of the reference's modules and as the recorded fixtures hold them
    assert state == list((OL.decoder_layout() if mod is new_decoder else OL.simple_decoder_layout()).keys())
    if mod is new_decoder:
        for f, k in (("model_b2s2.npz", "gradnorm_keys_decoder"), ("decoder_b2s9.npz", "gradnorm_keys")):
            assert [str(n) for n in np.load(os.path.join(GOLDEN, f))[k]] == sorted(params), f
    else:
        assert [k[3:] for k in np.load(os.path.join(GOLDEN, "simple_b2s2.npz")).keys() if k.startswith("gn/")] == params


TRUNK_METHODS = ("_init_weights", "_prepare", "_memory", "_check_lengths", "prepare_memory", "_stack", "_inference_pass",
                 "_inference_pass_cached", "forward_inference", "_build_trunk", "_teacher_forced", "forward_training")


def test_trunk_methods_are_defined_once():
    T = decoder_trunk.DecoderTrunk
    for name in TRUNK_METHODS:
        assert getattr(new_decoder.Decoder, name) is getattr(simple.Decoder, name) is getattr(T, name), name
        assert name not in vars(new_decoder.Decoder) and name not in vars(simple.Decoder), name
    for cls in (new_decoder.Decoder, simple.Decoder):
        assert "decode_mode" not in vars(cls) and cls.decode_mode == T.decode_mode == "recompute"
    # the trunk half of register is the trunk's; the simple decoder has no other half
    assert simple.Decoder.register is T.register and "register" in vars(new_decoder.Decoder)
    # the one switch between the two stacks
    assert new_decoder.Decoder.token_programs is True and simple.Decoder.token_programs is False and T.token_programs is False


@pytest.mark.parametrize("mod", [new_decoder, simple], ids=["new_decoder", "simple"])
def test_lengths_are_checked_before_the_weights_are_prepared(mod):
    dec = decoder_of(mod)
    calls = []
    dec._prepare = lambda: calls.append(1)
    n = torch.tensor([1, 1], dtype=torch.int32)
    dec.train()
    try:
        _check_order(dec, n)
    finally:
        del dec._prepare
        dec.eval()
    assert calls == []


def _check_order(dec, n):
    with pytest.raises(ValueError, match="inference"):
        dec.forward_inference(torch.zeros(2, 2, 256), 1, lengths=n)
    with pytest.raises(ValueError, match="inference"):
        dec.prepare_memory(torch.zeros(2, 1, 256), torch.zeros(2, 256), lengths=n)
    with pytest.raises(ValueError, match="inference"):
        dec(torch.zeros(2, 1, 256), torch.zeros(2, 256), lengths=n)
    dec.eval()
    for bad in (torch.tensor([1, 1]), torch.tensor([1, 1, 1], dtype=torch.int32)):
        with pytest.raises(ValueError, match="int32"):
            dec.forward_inference(torch.zeros(2, 2, 256), 1, lengths=bad)
    with pytest.raises(ValueError, match="positional table"):           # called directly: no check of lengths, but of the table
        dec._inference_pass(torch.zeros(1, 2, 256), dec.pos_encoding.pe.size(1) + 1)


# ---- the one check of a per-clip count tensor ----------------------------------------------------------------------------------------
def _refused(call, what, B, non_tensor):
    """call(t) must refuse int64, a wrong shape and (where the site always did) a non-tensor, naming the argument, int32 and (B,)."""
    bad = [torch.ones(B, dtype=torch.int64), torch.ones(B + 1, dtype=torch.int32), torch.ones(B, 1, dtype=torch.int32)]
    for t in bad + ([[1] * B] if non_tensor else []):
        with pytest.raises(ValueError, match="int32") as e:
            call(t)
        assert what in str(e.value) and f"({B},)" in str(e.value), str(e.value)


def test_len_tensor():
    n = torch.tensor([2, 1, 3], dtype=torch.int32)
    assert _lib.len_tensor(None, 3, "lengths") is None and _lib.len_tensor(None, 3, "lengths", training=True) is None
    assert _lib.len_tensor(n, 3, "lengths") is n
    every_other = torch.arange(6, dtype=torch.int32)[::2]
    assert _lib.len_tensor(every_other, 3, "lengths") is every_other
    c = _lib.len_tensor(every_other, 3, "lengths", contiguous=True)
    assert c.is_contiguous() and c.tolist() == [0, 2, 4]
    with pytest.raises(ValueError, match=r"call \.eval\(\) first"):
        _lib.len_tensor(n, 3, "lengths", training=True)
    with pytest.raises(ValueError, match="int32 device tensor"):           # a CPU tensor where the site asks for the device
        _lib.len_tensor(n, 3, "n_samples", device=True)
    _refused(lambda t: _lib.len_tensor(t, 3, "key_len"), "key_len", 3, True)


def test_every_site_refuses_what_is_not_int32_of_shape_B():
    """Each site that takes a per-clip count and reaches its check without a device, under the argument name it reports.  (The
    session's original_frames and n_samples, resample_batch, stft_sections and inverse_STFT_batch look for the device first; they
    go through the same len_tensor.)  ContentEncoder.forward made no such check before the trunk refactor."""
    import ast_amd
    B = 2
    sec, cls, ok = torch.zeros(B, 1, 2, 287, 597), torch.zeros(B, 256), torch.ones(B, dtype=torch.int32)
    sess = StyleTransferSession(torch.nn.Identity(), torch.nn.Identity(), use_graph=False)
    style, content = ast_amd.StyleEncoder().eval(), ast_amd.ContentEncoder().eval()
    dec, sdec = decoder_of(new_decoder), decoder_of(simple)
    x, w, b = torch.zeros(4, 256), torch.zeros(30, 256), torch.zeros(30)
    q, out = torch.zeros(B * 2, 256), torch.zeros(B, 1, 2, 287, 4)
    sites = [
        ("with n_sections, n_sections", True, lambda t: sess(sec, cls, n_sections=t)),
        ("n_samples", True, lambda t: cqt._n_samples_arg(t, B, 256, 287, 96)),
        ("n_sections", False, lambda t: U.sections2spectrogram_batch(out, 287, n_sections=t)),
        ("n_frames", False, lambda t: U.sections2spectrogram_batch(out, 287, n_sections=ok, n_frames=t)),
        ("lengths", True, lambda t: style(sec, lengths=t)),
        ("lengths", True, lambda t: content(sec, t)),
        ("lengths", False, lambda t: dec(torch.zeros(B, 1, 256), cls, lengths=t)),
        ("lengths", False, lambda t: sdec.prepare_memory(torch.zeros(B, 1, 256), cls, lengths=t)),
        ("lengths", False, lambda t: ops.big_out_linear(x, w, b, 2, t)),
        ("key_len", False, lambda t: ops.AttnCoreFn.forward(None, q, q, B, 4, 2, 2, 64, 0, 0, False, 0.0, t, 2)),
    ]
    with torch.no_grad():
        for what, non_tensor, call in sites:
            _refused(call, what, B, non_tensor)
        with pytest.raises(ValueError, match="int32"):                  # frontend_lengths takes B from the tensor itself
            U.frontend_lengths(torch.ones(B, dtype=torch.int64), 40000)
