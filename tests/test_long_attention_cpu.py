"""Attention past 16 tokens without a GPU: the CPU oracle against the reference decoder's fixture at B = 2, S = 9 (18 memory
tokens; tools/make_golden.py run_decoder_long), with the bounds tests/test_oracle_golden.py uses for the decoder, and the
argument checks of the four attention entry points, every one of which is refused before any launch."""
import math
import os
import re

import numpy as np
import pytest
import torch

from ast_amd import _lib, ops
from oracle import ast_oracle as O
from oracle import layout as L
from oracle import seeded_params as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000                                            # a 16-byte aligned non-null pointer; nothing dereferences it

torch.set_num_threads(min(8, os.cpu_count() or 1))


def _close(a, b, rtol, atol):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    scale = np.abs(b).max()
    assert np.allclose(a, b, rtol=rtol, atol=atol + rtol * scale), f"max abs err {np.abs(a - b).max()}, ref scale {scale}"


def _bias_before_norm(k):
    return bool(re.search(r"(conv_encoder\.(0|3|6|9)|spatial_projection\.0|conv_decoder\.(0|3|6|9))\.bias$", k))


def test_oracle_reproduces_the_reference_decoder_at_s9(golden_dir):
    g = np.load(os.path.join(golden_dir, "decoder_b2s9.npz"), allow_pickle=False)
    assert sp.layout_digest(L.LAYOUTS["decoder"]()) == bytes(g["layout_digest"]).decode()
    B, S = 2, 9
    sd = L.seeded_model_state("decoder")
    content, cls = sp.seeded_normal((B, S, 256), 5101), sp.seeded_normal((B, 256), 5102)
    y = sp.seeded_input(B, S, seed=5103, F=513)
    out = O.decoder_forward(sd, content, cls, O.Cfg(training=True, p_drop=0.0), y=y)
    rec = O.comprehensive_loss(out, y)
    rec["total_loss"].backward()
    assert out.shape == (B, S, 2, 287, 513)
    _close(out.detach()[:, :, :, ::23, ::29], g["out_sub"], 2e-4, 2e-5)
    for k in ("total_loss", "mse_loss", "mag_loss", "phase_loss", "temporal_loss", "spectral_loss"):
        assert math.isclose(float(rec[k]), float(g["rec_" + k]), rel_tol=1e-4, abs_tol=1e-6), k
    for k, v in zip((str(k) for k in g["gradnorm_keys"]), g["gradnorm_vals"]):
        gr = sd[k].grad
        got = -1.0 if gr is None else float(gr.norm())
        if v < 0:
            assert gr is None or got == 0.0, k
        elif _bias_before_norm(k):       # exactly 0 in real arithmetic: rounding noise on both sides
            assert got < 1e-3 and v < 1e-3, (k, got, v)
        else:
            assert math.isclose(got, v, rel_tol=5e-3, abs_tol=1e-6), (k, got, v)
    with torch.no_grad():                # eval-mode autoregressive decode, with the buffers the training forward updated
        ar = O.decoder_forward(sd, content, cls, O.Cfg(training=False), target_length=S)
    _close(ar[:, :, :, ::23, ::29], g["infer_sub"], 2e-4, 2e-5)


def test_cap_is_declared_and_mirrored():
    header = open(os.path.join(ROOT, "include", "ast_hip.h")).read()
    assert re.search(r"#define\s+AST_ATTN_MAX_L\s+1024\b", header)
    assert ops.ATTN_MAX_L == 1024
    assert "<=16 tokens" not in ops.AttnCoreFn.__doc__


def _fwd(lib, Lq=17, Lk=17, dh=64, H=4, q=FAKE, ld=None, p=0.0):
    ld = H * dh if ld is None else ld
    return lib.ast_attn_fwd_p(q, FAKE, FAKE, FAKE, FAKE, 2, H, Lq, Lk, dh, ld, ld, ld, 0, None, p, 0, None, None)


def _bwd(lib, Lq=17, Lk=17, dh=64, H=4, dq=FAKE, ld=None, p=0.0):
    ld = H * dh if ld is None else ld
    return lib.ast_attn_bwd_p(FAKE, FAKE, FAKE, FAKE, FAKE, dq, FAKE, FAKE, 2, H, Lq, Lk, dh, ld, ld, ld, None, p, 0, None, None)


@pytest.mark.parametrize("call,name", [(_fwd, b"ast_attn_fwd"), (_bwd, b"ast_attn_bwd")])
def test_attention_entries_refuse_bad_arguments(call, name):
    lib = _lib.lib()

    def refused(needle=None, **kw):
        assert call(lib, **kw) != 0, kw
        err = lib.ast_last_error()
        assert name in err and (needle is None or needle in err), (kw, err)

    refused(b"1024", Lq=1025)                                  # past the cap, and the message names it
    refused(b"1024", Lk=1025)
    refused(b"AST_ATTN_MAX_L", Lq=1025, Lk=1025)
    refused(b"dh", dh=65)                                      # wider than a wave's 64 lanes, at any length
    refused(b"dh", dh=65, Lq=4, Lk=4)
    refused(b"dh % 4", dh=30, Lq=17, Lk=17)                    # the tiled path loads 16 bytes at a time
    refused(b"dh % 4", dh=30, Lq=1, Lk=17)
    refused(Lq=0)
    refused(Lk=0)
    refused(b"16-byte", **({"q": FAKE + 4} if call is _fwd else {"dq": FAKE + 4}))
    refused(b"multiple of 4", ld=258)
    refused(p=1.0)
    refused(**({"q": None} if call is _fwd else {"dq": None}))


def test_plain_entries_share_the_checks():
    lib = _lib.lib()
    f = FAKE
    assert lib.ast_attn_fwd(f, f, f, f, f, 2, 4, 1025, 17, 64, 256, 256, 256, 0, None, None) != 0
    assert b"1024" in lib.ast_last_error()
    assert lib.ast_attn_bwd(f, f, f, f, f, f, f, f, 2, 4, 17, 17, 30, 120, 120, 120, None, None) != 0
    assert b"dh % 4" in lib.ast_last_error()
    assert lib.ast_attn_fwd(f, f, f, f, f, 2, 4, 17, 17, 65, 260, 260, 260, 0, None, None) != 0


def test_early_errors_name_the_limit():
    """More positions than a positional table holds, or more memory tokens than the attention core takes: a ValueError
    where the user called, not a C-ABI string from inside a layer."""
    import ast_amd
    pe = ast_amd.SinusoidalPositionalEncoding(256)
    pe(torch.zeros(1, 500, 256))
    with pytest.raises(ValueError, match="500 positions"):
        pe(torch.zeros(1, 501, 256))
    dec = ast_amd.Decoder()
    with pytest.raises(ValueError, match="1024"):
        dec._memory(torch.zeros(1, 513, 256), torch.zeros(1, 256))
    with pytest.raises(ValueError, match="500 positions"):
        dec._inference_pass(torch.zeros(1, 4, 256), target_length=501)
