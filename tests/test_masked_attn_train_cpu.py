"""Key-masked attention in training, without a GPU: the float64 restatement of the masked core (forward AND backward, explicit
0 / 1/(1-p) dropout mask, causal, the period rule, the clamp) that tests/test_gpu_masked_attn_train.py compares the kernels
against, checked here against torch.autograd on a dense float64 softmax with -inf scores; the cases, inputs and seeds of that
GPU test, with the check that an ignored mask would show on every one of them; and the host argument checks of
ast_attn_fwd_len_p / ast_attn_bwd_len_p with fake pointers (every bad call is refused before any launch)."""
import functools
import math

import pytest
import torch

from ast_amd import _lib

FAKE = 0x10000                                            # a 16-byte aligned non-null pointer; nothing dereferences it
B, H = 3, 4
GPU_TOL = 1e-4                                            # of the tensor's scale: tests/test_gpu_long_attention.py, test_gpu_ragged.py
P_DROP = 0.1

# (Lq, Lk, key_period, causal, dh, key_len)
CASES = [(3, 3, 3, False, 64, [3, 1, 2]),                 # misc.hip, ML = 4
         (8, 16, 8, False, 64, [8, 1, 2]),                # ML = 16, both halves of a memory
         (1, 6, 3, False, 64, [3, 1, 2]),                 # ML = 8, one query
         (9, 18, 9, False, 64, [9, 1, 2]),                # attn.hip: the second half starts inside key tile 0
         (17, 34, 17, False, 64, [17, 1, 2]),             # a boundary inside a key tile
         (33, 33, 33, True, 64, [33, 1, 2]),              # causal, whole key tiles masked
         (65, 130, 65, False, 64, [65, 1, 40]),           # whole key tiles masked, several query tiles, a boundary inside tile 2
         (17, 34, 17, False, 32, [17, 1, 2])]
CASE_IDS = [f"{c[0]}x{c[1]}p{c[2]}{'c' if c[3] else ''}dh{c[4]}" for c in CASES]


def live_keys(Lk, period, n):
    kl = min(max(int(n), 1), period)
    return [j for j in range(Lk) if j % period < kl]


@functools.lru_cache(maxsize=None)
def case_inputs(idx):
    """Seeded q (B*Lq, d), k, v (B*Lk, d), incoming gradient g (B*Lq, d) and a dropout mask (B, H, Lq, Lk) of 0 / 1/(1-p), float32.
    Shared by the CPU and the GPU tests; nobody writes to them."""
    Lq, Lk, period, causal, dh, _ = CASES[idx]
    gen = torch.Generator().manual_seed(4100 + idx)
    d = H * dh
    q, k, v, g = (torch.randn(n, d, generator=gen) for n in (B * Lq, B * Lk, B * Lk, B * Lq))
    keep = torch.rand(B, H, Lq, Lk, generator=gen) >= P_DROP
    mask = keep.float() * (1.0 / (1.0 - P_DROP))
    return q, k, v, g, mask


def masked_core_f64(q, k, v, g, Lq, Lk, dh, causal, key_len, period, mask=None):
    """The masked core and its gradients in float64, written out (no autograd): over the keys j of batch b with
    (j % period) < clamp(key_len[b], 1, period) only -- the other K / V rows are not read (NaN there is harmless), their probs,
    dk and dv are 0.  probs are those BEFORE dropout; mask (B, H, Lq, Lk) multiplies them on the way to o.
    q, g: (B*Lq, H*dh); k, v: (B*Lk, H*dh).  Returns dict(o, probs, dq, dk, dv)."""
    nb = q.shape[0] // Lq
    q, k, v, g = (t.detach().double().cpu() for t in (q, k, v, g))
    hs = lambda t, L: t.view(nb, L, H, dh).transpose(1, 2)                       # (B, H, L, dh)
    Q, K, V, G = hs(q, Lq), hs(k, Lk), hs(v, Lk), hs(g, Lq)
    o, dq = torch.zeros(nb, H, Lq, dh, dtype=torch.float64), torch.zeros(nb, H, Lq, dh, dtype=torch.float64)
    dk, dv = torch.zeros(nb, H, Lk, dh, dtype=torch.float64), torch.zeros(nb, H, Lk, dh, dtype=torch.float64)
    probs = torch.zeros(nb, H, Lq, Lk, dtype=torch.float64)
    scale = 1.0 / math.sqrt(dh)
    for b in range(nb):
        keys = torch.tensor(live_keys(Lk, period, key_len[b]))
        Kb, Vb = K[b][:, keys], V[b][:, keys]
        s = Q[b] @ Kb.transpose(-1, -2) * scale                                 # (H, Lq, nkeys)
        if causal:
            s = s.masked_fill(keys[None, None, :] > torch.arange(Lq)[None, :, None], float("-inf"))
        p = torch.exp(s - s.max(-1, keepdim=True).values)
        p = p / p.sum(-1, keepdim=True)
        m = torch.ones_like(p) if mask is None else mask[b].double()[:, :, keys]
        o[b] = (p * m) @ Vb
        dpm = (G[b] @ Vb.transpose(-1, -2)) * m                                 # d loss / d p
        ds = p * (dpm - (dpm * p).sum(-1, keepdim=True)) * scale
        probs[b][:, :, keys] = p
        dq[b] = ds @ Kb
        dk[b][:, keys] = ds.transpose(-1, -2) @ Q[b]
        dv[b][:, keys] = (p * m).transpose(-1, -2) @ G[b]
    flat = lambda t, L: t.transpose(1, 2).reshape(nb * L, H * dh)
    return dict(o=flat(o, Lq), probs=probs, dq=flat(dq, Lq), dk=flat(dk, Lk), dv=flat(dv, Lk))


def dense_autograd_f64(q, k, v, g, Lq, Lk, dh, causal, key_len, period, mask=None):
    """The same quantities from torch.autograd on a dense float64 softmax whose masked scores are -inf."""
    nb = q.shape[0] // Lq
    q, k, v = (t.detach().double().cpu().clone().requires_grad_(True) for t in (q, k, v))
    hs = lambda t, L: t.view(nb, L, H, dh).transpose(1, 2)
    s = hs(q, Lq) @ hs(k, Lk).transpose(-1, -2) / math.sqrt(dh)
    dead = torch.ones(nb, 1, 1, Lk, dtype=torch.bool)
    for b in range(nb):
        dead[b, 0, 0, live_keys(Lk, period, key_len[b])] = False
    s = s.masked_fill(dead, float("-inf"))
    if causal:
        s = s.masked_fill(torch.triu(torch.ones(Lq, Lk), diagonal=1).bool(), float("-inf"))
    probs = torch.softmax(s, dim=-1)
    P = probs if mask is None else probs * mask.double()
    o = (P @ hs(v, Lk)).transpose(1, 2).reshape(nb * Lq, H * dh)
    o.backward(g.detach().double().cpu())
    return dict(o=o.detach(), probs=probs.detach(), dq=q.grad, dk=k.grad, dv=v.grad)


def rel_err(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / max(b.abs().max().item(), 1e-12))


@functools.lru_cache(maxsize=None)
def case_reference(idx, dropout):
    """masked_core_f64 of case idx, computed once (nobody writes to it)."""
    Lq, Lk, period, causal, dh, key_len = CASES[idx]
    q, k, v, g, mask = case_inputs(idx)
    return masked_core_f64(q, k, v, g, Lq, Lk, dh, causal, key_len, period, mask if dropout else None)


# ---- the restatement itself -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [0, 1, 2, 3, 5], ids=[CASE_IDS[i] for i in (0, 1, 2, 3, 5)])
@pytest.mark.parametrize("dropout", [False, True], ids=["p0", "p0.1"])
def test_restatement_against_autograd(idx, dropout):
    Lq, Lk, period, causal, dh, key_len = CASES[idx]
    q, k, v, g, mask = case_inputs(idx)
    ref = dense_autograd_f64(q, k, v, g, Lq, Lk, dh, causal, key_len, period, mask if dropout else None)
    got = case_reference(idx, dropout)
    for n in ("o", "probs", "dq", "dk", "dv"):
        assert rel_err(got[n], ref[n]) < 1e-12, n


def test_restatement_mask_rules():
    """Masked probs, dk and dv are exactly 0; NaN in masked K / V rows reaches nothing; lengths are clamped to [1, period]; the
    period rule keeps both halves of a memory; full lengths are the plain core."""
    idx = 1
    Lq, Lk, period, causal, dh, key_len = CASES[idx]                            # (8, 16, 8), key_len [8, 1, 2]
    q, k, v, g, mask = case_inputs(idx)
    ref = case_reference(idx, True)
    kn, vn = k.clone().view(B, Lk, -1), v.clone().view(B, Lk, -1)
    for b in range(B):
        live = live_keys(Lk, period, key_len[b])
        dead = [j for j in range(Lk) if j not in live]
        assert live == [j for j in range(Lk) if j % 8 < key_len[b]]
        kn[b, dead] = float("nan"); vn[b, dead] = float("nan")
        assert (ref["probs"][b][:, :, dead] == 0).all()
        assert (ref["dk"].view(B, Lk, -1)[b, dead] == 0).all() and (ref["dv"].view(B, Lk, -1)[b, dead] == 0).all()
        assert torch.allclose(ref["probs"][b].sum(-1), torch.ones(H, Lq, dtype=torch.float64))
    nan = masked_core_f64(q, kn.view(B * Lk, -1), vn.view(B * Lk, -1), g, Lq, Lk, dh, causal, key_len, period, mask)
    for n in ref:
        assert torch.equal(nan[n], ref[n]), n
    a = masked_core_f64(q, k, v, g, Lq, Lk, dh, causal, [0, -5, 100], period, mask)
    b_ = masked_core_f64(q, k, v, g, Lq, Lk, dh, causal, [1, 1, 8], period, mask)
    for n in a:
        assert torch.equal(a[n], b_[n]), n
    full = masked_core_f64(q, k, v, g, Lq, Lk, dh, causal, [8, 8, 8], period, mask)
    dense = dense_autograd_f64(q, k, v, g, Lq, Lk, dh, causal, [8, 8, 8], period, mask)
    for n in full:
        assert rel_err(full[n], dense[n]) < 1e-12, n


@pytest.mark.parametrize("idx", range(len(CASES)), ids=CASE_IDS)
@pytest.mark.parametrize("dropout", [False, True], ids=["p0", "p0.1"])
def test_seeds_show_an_ignored_mask(idx, dropout):
    """The GPU test asserts that the UNMASKED backward on the same padded inputs misses the masked reference by more than its
    tolerance.  Here, in float64: with these seeds the unmasked dq / dk / dv are at least 10 x that tolerance away."""
    Lq, Lk, period, causal, dh, key_len = CASES[idx]
    q, k, v, g, mask = case_inputs(idx)
    ref = case_reference(idx, dropout)
    un = masked_core_f64(q, k, v, g, Lq, Lk, dh, causal, [period] * B, period, mask if dropout else None)
    for n in ("dq", "dk", "dv"):
        assert rel_err(un[n], ref[n]) >= 10 * GPU_TOL, (n, rel_err(un[n], ref[n]))


# ---- host argument checks ---------------------------------------------------------------------------------------------------------
def _call(lib, entry, Lq=3, Lk=6, period=3, key_len=FAKE, dh=64, nh=4, first=FAKE, last=FAKE, ld=None, p=0.1, drop=None):
    ld = nh * dh if ld is None else ld
    if entry == "ast_attn_fwd_len_p":
        return lib.ast_attn_fwd_len_p(first, FAKE, FAKE, last, FAKE, 2, nh, Lq, Lk, dh, ld, ld, ld, 0, key_len, period, drop, p, 7, None,
                                      None)
    return lib.ast_attn_bwd_len_p(first, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, last, 2, nh, Lq, Lk, dh, ld, ld, ld, key_len, period, drop,
                                  p, 7, None, None)


@pytest.mark.parametrize("entry", ["ast_attn_fwd_len_p", "ast_attn_bwd_len_p"])
def test_masked_training_entries_refuse_bad_arguments(entry):
    lib = _lib.lib()

    def refused(needle, **kw):
        assert _call(lib, entry, **kw) != 0, kw
        err = lib.ast_last_error()
        assert entry.encode() in err and needle in err, (kw, err)

    refused(b"key_period", period=0)
    refused(b"key_period", period=7)                           # > Lk
    refused(b"key_period", period=4)                           # Lk % key_period != 0
    refused(b"key_period", period=-3)
    refused(b"key_period", Lq=17, Lk=34, period=16)
    refused(b"key_len", key_len=None)
    refused(b"key_len", key_len=None, Lq=17, Lk=34, period=17)
    refused(b"p <", p=1.0)
    refused(b"p <", p=-0.1)
    refused(b"p <", p=float("nan"))
    refused(b"p <", p=1.5, Lq=17, Lk=34, period=17)
    # everything the unmasked entries check, on both paths
    refused(b"bad args", first=None)
    refused(b"bad args", last=None)
    refused(b"dh", dh=65)
    refused(b"1<=L", Lq=0)
    refused(b"1<=L", Lk=-1, period=1)
    refused(b"1024", Lq=1, Lk=1026, period=513)
    refused(b"dh % 4", dh=30, Lq=17, Lk=34, period=17)
    refused(b"16-byte", first=FAKE + 4, Lq=1, Lk=34, period=17)
    refused(b"16-byte", last=FAKE + 4, Lq=17, Lk=34, period=17)
    refused(b"multiple of 4", ld=258, Lq=17, Lk=34, period=17)
    refused(b"row strides", ld=128, Lq=17, Lk=34, period=17)


def test_valid_masked_training_calls_pass_the_checks_up_to_the_launch():
    """Without a device a valid call gets past every argument check and fails in the launch, with the runtime's message."""
    if torch.cuda.is_available():
        return                                                  # with a device the valid calls run in tests/test_gpu_masked_attn_train.py
    lib = _lib.lib()
    for entry in ("ast_attn_fwd_len_p", "ast_attn_bwd_len_p"):
        for kw in (dict(), dict(Lq=8, Lk=16, period=8, drop=FAKE), dict(Lq=1, Lk=34, period=17, p=0.0), dict(Lq=17, Lk=17, period=17, dh=32)):
            assert _call(lib, entry, **kw) != 0, (entry, kw)
            err = lib.ast_last_error()
            for word in (b"bad args", b"needs", b"NULL", b"at most", b"16-byte"):
                assert word not in err, (entry, kw, err)


def test_ops_and_layers_expose_the_masked_training_path():
    """MaskedAttnFn exists next to AttnCoreFn, and the refusals of the inference-only pieces are still there."""
    from ast_amd import ops
    assert issubclass(ops.MaskedAttnFn, torch.autograd.Function)
    with pytest.raises(ValueError, match="key_len"):
        ops.MaskedAttnFn.apply(torch.zeros(3, 8), torch.zeros(3, 16), 1, 1, 3, 3, 8, 0, 8, False, 0.0, None, 3)
    t = torch.zeros(2, 2, requires_grad=True)
    with pytest.raises(RuntimeError, match="inference only"):
        ops.require_inference(t)
    with pytest.raises(ValueError, match="inference"):
        _lib.len_tensor(torch.zeros(2, dtype=torch.int32), 2, "lengths", training=True)
