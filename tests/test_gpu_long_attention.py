"""Attention past 16 tokens (csrc/attn.hip: 17 .. AST_ATTN_MAX_L = 1024 tokens, tiles of 16 queries x 16 keys on exact-f32
MFMA), from the core through MHA, the decoder, the inference session and the trainer at S = 9 sections (18 memory tokens).

Tolerances are the project's own: 1e-4 of the tensor scale for the core against the softmax formula in float64 (as
test_attention_dropout_drawn_in_kernel), 2e-4 through MHA (test_mha), 1e-3 / 1e-2 against oracle and fixture
(test_gpu_models.py).  The float64 reference of every core case is computed once per case and shared by its checks."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import ast_amd
    from ast_amd import config, layers as AL, ops
    from ast_amd._lib import lib
from oracle import ast_oracle as O
from oracle import layout as OL
from oracle import seeded_params as sp

DEV = "cuda"


def rel_err(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / max(b.abs().max().item(), 1e-12))


def host_dropout_mask(seed, counter, n, p):
    """csrc/ast_common.h dropout_keep on the host (the recipe of tests/test_gpu_ops.py, vectorised in uint64)."""
    with np.errstate(over="ignore"):
        def mix(z):
            z = z + np.uint64(0x9E3779B97F4A7C15)
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            return z ^ (z >> np.uint64(31))
        base = mix(np.uint64(seed) ^ mix(np.uint64(counter)))
        r = (mix(base + np.arange(n, dtype=np.uint64)) >> np.uint64(40)).astype(np.float32)
    keep = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    return torch.from_numpy(np.where(r * np.float32(1.0 / 16777216.0) >= np.float32(p), keep, np.float32(0.0)).astype(np.float32))


def reference(q, k, v, g, B, H, Lq, Lk, dh, causal, mask=None):
    """softmax(Q K^T / sqrt(dh) + causal) (o mask) V and its gradients in float64.  q, g: (B*Lq, d); k, v: (B*Lk, d)."""
    q, k, v = (t.detach().double().cpu().clone().requires_grad_(True) for t in (q, k, v))
    Q = q.view(B, Lq, H, dh).transpose(1, 2)
    K = k.view(B, Lk, H, dh).transpose(1, 2)
    V = v.view(B, Lk, H, dh).transpose(1, 2)
    s = Q @ K.transpose(-1, -2) / math.sqrt(dh)
    if causal:
        s = s.masked_fill(torch.triu(torch.ones(Lq, Lk), diagonal=1).bool(), float("-inf"))
    probs = torch.softmax(s, dim=-1)
    P = probs if mask is None else probs * mask.double()
    o = (P @ V).transpose(1, 2).reshape(B * Lq, H * dh)
    o.backward(g.double().cpu())
    return dict(o=o.detach(), probs=probs.detach(), dq=q.grad, dk=k.grad, dv=v.grad)


def run_core(B, H, Lq, Lk, dh, causal, layout="kv", p=0.0, seed=0, backward=True):
    """AttnCoreFn on seeded inputs in one of MHA's two layouts: "kv" = q (B*Lq, d) and K | V as column offsets of one
    (B*Lk, 2d) buffer (cross-attention, the cached decode step); "qkv" = q | k | v of one (B*L, 3d) buffer (self-attention)."""
    gen = torch.Generator().manual_seed(1000 + 31 * Lq + Lk + seed)
    d = H * dh
    g = torch.randn(B * Lq, d, generator=gen)
    if layout == "qkv":
        assert Lq == Lk
        buf = torch.randn(B * Lq, 3 * d, generator=gen).to(DEV).requires_grad_(True)
        o = ops.AttnCoreFn.apply(buf, buf, B, H, Lq, Lk, dh, d, 2 * d, causal, p)
        parts = lambda t: (t[:, :d], t[:, d:2 * d], t[:, 2 * d:])
    else:
        q = torch.randn(B * Lq, d, generator=gen).to(DEV).requires_grad_(True)
        kv = torch.randn(B * Lk, 2 * d, generator=gen).to(DEV).requires_grad_(True)
        o = ops.AttnCoreFn.apply(q, kv, B, H, Lq, Lk, dh, 0, d, causal, p)
    probs = o.grad_fn.saved_tensors[2]
    got = dict(o=o.detach().clone(), probs=probs.detach().clone())
    if backward:
        o.backward(g.to(DEV))
    if layout == "qkv":
        qi, ki, vi = (t.detach().contiguous() for t in parts(buf))
        if backward:
            got["dq"], got["dk"], got["dv"] = (t.clone() for t in parts(buf.grad))
    else:
        qi, ki, vi = q.detach(), kv.detach()[:, :d].contiguous(), kv.detach()[:, d:].contiguous()
        if backward:
            got["dq"], got["dk"], got["dv"] = q.grad.clone(), kv.grad[:, :d].clone(), kv.grad[:, d:].clone()
    return got, (qi, ki, vi, g)


def check_core(B, H, Lq, Lk, dh, causal, layout="kv", backward=True):
    got, (q, k, v, g) = run_core(B, H, Lq, Lk, dh, causal, layout, backward=backward)
    ref = reference(q, k, v, g, B, H, Lq, Lk, dh, causal)
    errs = {n: rel_err(got[n], ref[n]) for n in got}
    print(f"core B={B} H={H} Lq={Lq} Lk={Lk} dh={dh} causal={causal} {layout}: " + " ".join(f"{n}={e:.2e}" for n, e in errs.items()))
    assert set(errs) == ({"o", "probs", "dq", "dk", "dv"} if backward else {"o", "probs"})
    for n, e in errs.items():
        assert e < 1e-4, (n, e)
    if causal:
        assert float(got["probs"].triu(1).abs().max()) == 0.0


CASES = [(2, 16, 16, True),       # still the <= 16-token kernel: boundary and regression
         (2, 17, 17, True),       # first long self-attention
         (2, 9, 18, False),       # cross-attention at S = 9: ragged in both dimensions
         (2, 33, 33, True),
         (2, 64, 128, False),     # full tiles only
         (2, 65, 130, False),     # one past full tiles
         (1, 5, 1024, False),     # the cap
         (1, 200, 400, False)]


@pytest.mark.parametrize("B,Lq,Lk,causal", CASES)
def test_core_against_float64(B, Lq, Lk, causal):
    check_core(B, 4, Lq, Lk, 64, causal, layout="qkv" if causal else "kv")


@pytest.mark.parametrize("Lk", [17, 34])
def test_decode_step_forward(Lk):
    """Lq = 1: the KV-cached decode step against its cache (17 tokens) and against the memory (2 * 17)."""
    check_core(2, 4, 1, Lk, 64, False, backward=False)


def test_head_width_32():
    check_core(2, 4, 17, 34, 32, False)


def test_both_mha_layouts_non_causal():
    """K | V of one (B*Lk, 2d) buffer and q | k | v of one (B*L, 3d) buffer (the gradient of the latter is ONE buffer too)."""
    check_core(2, 4, 34, 34, 64, False, layout="qkv")
    check_core(2, 4, 34, 34, 64, False, layout="kv")


def test_nothing_outside_the_outputs_is_written():
    """o, probs, dq, dk, dv inside one NaN-filled buffer with guard bands: the guards stay NaN, the outputs are finite."""
    B, H, Lq, Lk, dh = 2, 4, 17, 35, 64
    d = H * dh
    gen = torch.Generator().manual_seed(77)
    q, k, v, g = (torch.randn(n, d, generator=gen).to(DEV) for n in (B * Lq, B * Lk, B * Lk, B * Lq))
    sizes = dict(o=B * Lq * d, probs=B * H * Lq * Lk, dq=B * Lq * d, dk=B * Lk * d, dv=B * Lk * d)
    GUARD = 1024
    off, at = GUARD, {}
    for n, sz in sizes.items():
        at[n] = off
        off += (sz + 3) // 4 * 4 + GUARD                    # 16-byte aligned starts
    buf = torch.full((off,), float("nan"), device=DEV)
    view = {n: buf[at[n]:at[n] + sizes[n]] for n in sizes}
    a = lambda n: view[n].data_ptr()
    ops.check(lib().ast_attn_fwd_p(q.data_ptr(), k.data_ptr(), v.data_ptr(), a("o"), a("probs"), B, H, Lq, Lk, dh, d, d, d, 0, None,
                                   0.0, 0, None, ops.stream()), "ast_attn_fwd")
    ops.check(lib().ast_attn_bwd_p(g.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(), a("probs"), a("dq"), a("dk"), a("dv"),
                                   B, H, Lq, Lk, dh, d, d, d, None, 0.0, 0, None, ops.stream()), "ast_attn_bwd")
    torch.cuda.synchronize()
    inside = torch.zeros(off, dtype=torch.bool, device=DEV)
    for n in sizes:
        inside[at[n]:at[n] + sizes[n]] = True
        assert bool(torch.isfinite(view[n]).all()), n
    assert bool(torch.isnan(buf[~inside]).all())
    ref = reference(q, k, v, g, B, H, Lq, Lk, dh, False)
    for n in sizes:
        assert rel_err(view[n].view(ref[n].shape), ref[n]) < 1e-4, n


def test_dropout_drawn_in_kernel():
    """p = 0.3 at (17, 34): forward and backward draw the same mask, rebuilt here on the host from (seed, counter, index)."""
    B, H, Lq, Lk, dh = 2, 4, 17, 34, 64
    ops._DropState.calls = 3000
    got, (q, k, v, g) = run_core(B, H, Lq, Lk, dh, False, p=0.3)
    mask = host_dropout_mask(ops._DropState.seed + 7919 * 3001, int(ops._DropState.counter.item()), B * H * Lq * Lk, 0.3).view(B, H, Lq, Lk)
    assert 0.2 < float((mask == 0).float().mean()) < 0.4
    ref = reference(q, k, v, g, B, H, Lq, Lk, dh, False, mask=mask)
    for n in ("o", "probs", "dq", "dk", "dv"):                # probs are saved BEFORE dropout
        assert rel_err(got[n], ref[n]) < 1e-4, n


def test_two_runs_are_bitwise_equal():
    a, _ = run_core(2, 4, 65, 130, 64, False)
    b, _ = run_core(2, 4, 65, 130, 64, False)
    for n in ("o", "probs", "dq", "dk", "dv"):
        assert torch.equal(a[n], b[n]), n


@pytest.mark.parametrize("cross,causal,Lq,Lk", [(False, True, 17, 17), (True, False, 9, 18)])
def test_mha_past_16_tokens(cross, causal, Lq, Lk):
    """layers.MHA against nn.MultiheadAttention, as tests/test_gpu_ops.py::test_mha."""
    torch.manual_seed(8)
    d, h, B = 256, 4, 3
    m = nn.MultiheadAttention(d, h, dropout=0.0, batch_first=True).to(DEV)
    with torch.no_grad():
        m.in_proj_bias.normal_(0, 0.1); m.out_proj.bias.normal_(0, 0.1)
    ref = nn.MultiheadAttention(d, h, dropout=0.0, batch_first=True)
    ref.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
    x, mem = torch.randn(B, Lq, d), torch.randn(B, Lk, d)
    xr, memr = x.clone().requires_grad_(True), mem.clone().requires_grad_(True)
    mask = torch.triu(torch.ones(Lq, Lq), diagonal=1).bool() if causal else None
    yr, _ = ref(xr, memr if cross else xr, memr if cross else xr, attn_mask=mask, need_weights=False)
    gy = torch.randn_like(yr)
    yr.backward(gy)
    config.set_compute_dtype(torch.float32)
    bank = AL.WeightBank()
    att = AL.MHA(bank, m, cross=cross)
    bank.prepare(True)
    xh, memh = x.to(DEV).requires_grad_(True), mem.to(DEV).requires_grad_(True)
    y = att(xh, memh if cross else None, True, 0.0, causal=causal)
    assert rel_err(y, yr) < 2e-4
    y.backward(gy.to(DEV))
    assert rel_err(xh.grad, xr.grad) < 2e-4
    if cross:
        assert rel_err(memh.grad, memr.grad) < 2e-4
    assert rel_err(m.in_proj_weight.grad, ref.in_proj_weight.grad) < 2e-4
    assert rel_err(m.in_proj_bias.grad, ref.in_proj_bias.grad) < 2e-4
    assert rel_err(m.out_proj.weight.grad, ref.out_proj.weight.grad) < 2e-4


# ---- model level: S = 9 sections and more ---------------------------------------------------------------------------------------
def _seeded(tag, ctor, train_mode):
    m = ctor()
    m.load_state_dict(sp.seeded_state_dict(m.state_dict(), tag=tag))
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
        if isinstance(mod, torch.nn.MultiheadAttention):
            mod.dropout = 0.0
    m = m.to(DEV)
    return m.train() if train_mode else m.eval()


def _bias_before_norm(k):
    import re
    return bool(re.search(r"(conv_encoder\.(0|3|6|9)|spatial_projection\.0|conv_decoder\.(0|3|6|9))\.bias$", k))


def test_decoder_against_reference_fixture_at_s9(golden_dir):
    """Teacher-forced forward + backward, then the eval-mode autoregressive decode, at B = 2, S = 9 against the real
    reference decoder (tests/golden/decoder_b2s9.npz, tools/make_golden.py run_decoder_long).  Gradient norms: 1e-2 wherever
    the reference norm exceeds 1e-6, except the nine conv biases in front of a Batch/InstanceNorm: their gradient is exactly 0
    in real arithmetic, the reference holds rounding noise there (up to 3.9e-6 for conv_encoder.0.bias), and a relative bound
    on noise means nothing; they are bounded by 1e-3 absolutely, as in tests/test_oracle_golden.py."""
    g = np.load(os.path.join(golden_dir, "decoder_b2s9.npz"), allow_pickle=False)
    config.set_compute_dtype(torch.float32)
    B, S = 2, 9
    dec = _seeded("decoder", ast_amd.Decoder, True)
    assert sp.layout_digest(dec.state_dict()) == bytes(g["layout_digest"]).decode()
    content, cls = sp.seeded_normal((B, S, 256), 5101).to(DEV), sp.seeded_normal((B, 256), 5102).to(DEV)
    y = sp.seeded_input(B, S, seed=5103, F=513).to(DEV)
    out = dec(content, cls, y=y)
    rec = ast_amd.compute_comprehensive_loss(out, y)
    rec["total_loss"].backward()
    torch.cuda.synchronize()
    assert rel_err(out[:, :, :, ::23, ::29], g["out_sub"]) < 1e-3
    for k in ("total_loss", "mse_loss", "mag_loss", "phase_loss", "temporal_loss", "spectral_loss"):
        assert math.isclose(float(rec[k]), float(g["rec_" + k]), rel_tol=1e-3, abs_tol=1e-6), k
    params, bad, checked = dict(dec.named_parameters()), [], 0
    for k, v in zip((str(k) for k in g["gradnorm_keys"]), g["gradnorm_vals"]):
        got = 0.0 if params[k].grad is None else float(params[k].grad.norm())
        if _bias_before_norm(k):
            ok = got < 1e-3 and v < 1e-3
        elif v > 1e-6:
            ok, checked = math.isclose(got, v, rel_tol=1e-2), checked + 1
        else:
            ok = True
        if not ok:
            bad.append((k, got, float(v)))
    assert not bad, bad[:8]
    assert checked >= 100
    dec.eval()
    with torch.no_grad():
        ar = dec(content, cls, target_length=S)
    assert rel_err(ar[:, :, :, ::23, ::29], g["infer_sub"]) < 1e-3


@pytest.mark.parametrize("B,S", [(2, 9), (1, 17)])
def test_kv_cached_decode_past_16_tokens(B, S):
    """As test_kv_cached_decode_equals_recompute.  S = 9: 18 memory tokens; S = 17: the decoder's self-attention passes 16
    tokens as well (causal 17 x 17 in the recompute loop, 1 x 17 against the cache)."""
    config.set_compute_dtype(torch.float32)
    dec = _seeded("decoder", ast_amd.Decoder, False)
    content = sp.seeded_normal((B, S, 256), 991).to(DEV)
    cls = sp.seeded_normal((B, 256), 992).to(DEV)
    with torch.no_grad():
        dec.decode_mode = "recompute"
        ref = dec(content, cls, target_length=S)
        dec.decode_mode = "kv_cache"
        try:
            got = dec(content, cls, target_length=S)
        finally:
            dec.decode_mode = "recompute"
    assert ref.shape == (B, S, 2, 287, 513) and float(ref.abs().max()) > 0
    assert rel_err(got, ref) < 1e-5
    sd = OL.seeded_model_state("decoder", requires_grad=False)
    oo = O.decoder_forward(sd, content.cpu(), cls.cpu(), O.Cfg(training=False), target_length=S)
    assert rel_err(got, oo) < 1e-3


def test_inference_session_at_s9():
    """StyleTransferSession on a 9-section clip (about 21 s), eager and as a replayed graph, against the oracle pipeline."""
    from ast_amd.infer import StyleTransferSession
    config.set_compute_dtype(torch.float32)
    B, S = 1, 9
    content_enc, dec = _seeded("content", ast_amd.ContentEncoder, False), _seeded("decoder", ast_amd.Decoder, False)
    sections = sp.seeded_input(B, S).to(DEV)
    cls = sp.seeded_normal((B, 256), 5202).to(DEV)
    wav_e, out_e = StyleTransferSession(content_enc, dec, use_graph=False)(sections, cls)
    wav_e, out_e = wav_e.clone(), out_e.clone()
    sess = StyleTransferSession(content_enc, dec, use_graph=True)
    wav_g, out_g = sess(sections, cls)
    wav_g, out_g = wav_g.clone(), out_g.clone()
    wav_g2, _ = sess(sections, cls)                                    # a second call replays the captured graph
    torch.cuda.synchronize()
    T = 8 * 191 + 287
    assert wav_e.shape == (B, 256 * (T - 1)) and wav_g.shape == wav_e.shape and out_e.shape == (B, S, 2, 287, 513)
    assert bool(torch.isfinite(wav_e).all()) and float(wav_e.abs().max()) > 0
    assert rel_err(out_g, out_e) < 1e-5 and rel_err(wav_g, wav_e) < 1e-5 and rel_err(wav_g2, wav_e) < 1e-5
    sds = {t: OL.seeded_model_state(t, requires_grad=False) for t in ("content", "decoder")}
    cfg = O.Cfg(training=False)
    with torch.no_grad():
        co = O.content_encoder_forward(sds["content"], sections.cpu(), cfg)
        oo = O.decoder_forward(sds["decoder"], co, cls.cpu(), cfg, target_length=S)
    assert rel_err(out_e, oo) < 1e-3


def _train_run(steps, **cfg):
    from ast_amd import train
    ast_amd.set_compute_dtype(torch.float32)
    tr = train.Trainer(train.TrainConfig(dropout=False, **cfg), seed=7)
    x, labels = train.synthetic_batch(2, 9, "cuda:0", seed=3)
    hist = []
    for _ in range(steps):
        out = tr.step(x, labels)
        torch.cuda.synchronize()
        hist.append({k: v.detach().clone() for k, v in out.items()})
    return hist, tr.G.flat_p.detach().clone(), tr.D.flat_p.detach().clone()


def test_trainer_at_s9_deterministic_and_default():
    """Trainer.step at B = 2, S = 9: two fresh deterministic Trainers agree bitwise after 2 steps (losses and parameters),
    the graph-replayed step is the eager step bit for bit, and the default-mode step computes the same step within the
    noise model test_default_and_deterministic_compute_the_same_step uses (tests/test_gpu_trainer.py _noise_tolerances)."""
    from test_gpu_trainer import _assert_close_hist, _noise_tolerances
    a, ga, da = _train_run(2, deterministic=True)
    b, gb, db = _train_run(2, deterministic=True)
    for la, lb in zip(a, b):
        assert la.keys() == lb.keys()
        for k in la:
            assert torch.equal(la[k], lb[k]), (k, float(la[k]), float(lb[k]))
    assert torch.equal(ga, gb) and torch.equal(da, db)
    assert all(math.isfinite(float(v)) for l in a for v in l.values())
    e, ge, de = _train_run(1, deterministic=True, use_graph=False)
    for k in e[0]:
        assert torch.equal(e[0][k], a[0][k]), ("graph replay against eager", k, float(e[0][k]), float(a[0][k]))
    f = lambda hist: [{k: float(v) for k, v in l.items()} for l in hist]
    d1, d2 = f(_train_run(1, use_graph=False)[0]), f(_train_run(1, use_graph=False)[0])
    assert all(math.isfinite(v) for v in d1[0].values())
    _assert_close_hist(f(e), d1, _noise_tolerances(d1, d2), "deterministic vs default at S = 9")
