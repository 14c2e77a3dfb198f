"""SimpleDecoder_TransformerOnly at inference without a GPU: the host checks of ast_bign_gemm_len (every call is refused before
any launch), the refusals of the Python layer, and the oracle's word that the inputs of the device tests show a missing mask."""
import functools
import os
import re

import pytest
import torch

from ast_amd import _lib, ops
from oracle import ast_oracle as O
from oracle import layout as OL
from test_ragged_cpu import N_SHORT, short_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000                                            # a 16-byte aligned non-null pointer; nothing dereferences it
NAME = "ast_bign_gemm_len"


def test_symbol_is_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "ast_hip.h")).read()
    assert NAME in _lib.EXPORTS and NAME in _lib._SIGS
    getattr(_lib.lib(), NAME)
    assert re.search(r"\b%s\(" % NAME, header)
    assert re.search(r"#define\s+AST_BIGN_MAX_ROWS\s+4096\b", header)
    assert ops.BIGN_MAX_ROWS == 4096 and ops.WIDE_MAX_ROWS == 1024


def test_bign_gemm_len_refuses_bad_arguments():
    lib = _lib.lib()
    f = FAKE
    call = lambda x=f, w=f, y=f, M=9, N=30, K=256, ldw=256, ldy=30, S=3, n=f: lib.ast_bign_gemm_len(x, w, None, y, M, N, K, ldw, ldy, S, n, None)
    bad = (dict(x=None), dict(w=None), dict(y=None), dict(M=0, S=1), dict(M=4097, S=1), dict(S=0), dict(M=10), dict(N=0),
           dict(K=254), dict(K=0), dict(K=2048, ldw=2048), dict(ldw=258), dict(ldw=128), dict(ldy=29), dict(x=f + 4), dict(w=f + 8),
           dict(N=16 * 65535 + 1, ldy=16 * 65535 + 1), dict(n=f + 2))
    for kw in bad:
        assert call(**kw) != 0, kw
        assert NAME.encode() in lib.ast_last_error(), (kw, lib.ast_last_error())


@pytest.fixture
def simple_decoder():
    from ast_amd.SimpleDecoder_TransformerOnly import Decoder
    return Decoder()


def test_lengths_are_refused_in_training_mode_and_as_int64(simple_decoder):
    n = torch.tensor([1, 1], dtype=torch.int32)
    dec = simple_decoder.train()
    with pytest.raises(ValueError, match="inference"):
        dec(torch.zeros(2, 1, 256), torch.zeros(2, 256), y=torch.zeros(2, 1, 2, 287, 513), lengths=n)
    with pytest.raises(ValueError, match="inference"):
        dec.prepare_memory(torch.zeros(2, 1, 256), torch.zeros(2, 256), lengths=n)
    with pytest.raises(ValueError, match="inference"):
        dec.forward_inference(torch.zeros(2, 2, 256), 1, lengths=n)
    dec.eval()
    with pytest.raises(ValueError, match="int32"):
        dec(torch.zeros(2, 1, 256), torch.zeros(2, 256), lengths=torch.tensor([1, 1]))
    with pytest.raises(ValueError, match="int32"):
        dec(torch.zeros(2, 1, 256), torch.zeros(2, 256), lengths=torch.tensor([1, 1, 1], dtype=torch.int32))


def test_limits_are_value_errors(simple_decoder):
    """2 Sc memory tokens past the attention core, and a target_length past the positional table: refused before any launch."""
    dec = simple_decoder.eval()
    dec._prepare = lambda: None
    with pytest.raises(ValueError, match="memory tokens"):
        dec(torch.zeros(1, ops.ATTN_MAX_L // 2 + 1, 256), torch.zeros(1, 256))
    with pytest.raises(ValueError, match="positional table"):
        dec._inference_pass(torch.zeros(1, 2, 256), dec.pos_encoding.pe.size(1) + 1)
    assert type(dec).decode_mode == "recompute"


def test_big_out_linear_is_inference_only():
    x, w, b = torch.zeros(4, 256, requires_grad=True), torch.zeros(30, 256), torch.zeros(30)
    with pytest.raises(RuntimeError, match="inference only"):
        ops.big_out_linear(x, w, b, 2)
    with pytest.raises(RuntimeError, match="inference only"):
        ops.big_out_linear(x.detach(), w.requires_grad_(), b, 2)
    with torch.no_grad(), pytest.raises(RuntimeError, match="device tensors"):      # past the grad check: no CPU path
        ops.big_out_linear(x, w, b, 2)
    with torch.no_grad(), pytest.raises(ValueError, match="whole number"):
        ops.big_out_linear(x, w, b, 3)
    with torch.no_grad(), pytest.raises(ValueError, match="int32"):
        ops.big_out_linear(x, w, b, 2, torch.tensor([1, 1]))
    with torch.no_grad(), pytest.raises(RuntimeError, match="4096"):
        ops.big_out_linear(torch.zeros(4097, 256), w, b, 1)


# ---- inputs and oracle references of the model test (tests/test_gpu_simple_infer.py) --------------------------------------------------
# The clips are test_ragged_cpu.short_inputs(): (3, 3, 256) seeded-normal content rows, rows s >= n_b seeded noise of the same
# scale as the real ones, so that without lengths they leak in.
@functools.lru_cache(maxsize=None)
def simple_solo_oracle():
    """The CPU oracle's simple-decoder output of every clip alone, on its own rows of the content embeddings."""
    _, cls, rows = short_inputs()
    sd = OL.seeded_model_state("simple_decoder", requires_grad=False)
    with torch.no_grad():
        return [O.simple_decoder_forward(sd, rows[b:b + 1, :n], cls[b:b + 1], O.Cfg(training=False), target_length=n)
                for b, n in enumerate(N_SHORT)]


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def test_seeds_show_a_missing_mask_simple():
    """The device test asserts that the padded batch WITHOUT lengths misses the 1e-3 bound by 10 x on the shorter clips.  Here the
    oracle says these inputs make it so with room to spare: more than 100 x the bound on clips 1 and 2 (measured: 0.21 / 0.13),
    while the full-length clip does not depend on its neighbours."""
    _, cls, rows = short_inputs()
    sd = OL.seeded_model_state("simple_decoder", requires_grad=False)
    with torch.no_grad():
        padded = O.simple_decoder_forward(sd, rows, cls, O.Cfg(training=False), target_length=3)
    gaps = [_rel(padded[b:b + 1, :n], simple_solo_oracle()[b]) for b, n in enumerate(N_SHORT)]
    print("simple decoder, padded batch without lengths against each clip alone:", gaps)
    assert gaps[0] < 1e-5 and min(gaps[1:]) > 100 * 1e-3, gaps
