"""Key-masked attention in training on the GPU: ast_attn_fwd_len_p / ast_attn_bwd_len_p against the float64 restatement of
tests/test_masked_attn_train_cpu.py (same cases, inputs and seeds), the exact properties of the mask, full lengths against the
unmasked kernels bit for bit, and the transformer layers on a padded batch against each clip run alone on the unmasked path.

Tolerances are the project's own: 1e-4 of the tensor's scale for the core against float64 (tests/test_gpu_long_attention.py,
tests/test_gpu_ragged.py), 2e-3 relative / 2e-4 absolute for the f32 layers (tests/test_gpu_validation.py REL, ABS)."""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import ast_amd
    from ast_amd import config, layers as AL, ops, tokprog
    from ast_amd._lib import lib
from test_masked_attn_train_cpu import (B, CASE_IDS, CASES, GPU_TOL, H, P_DROP, case_inputs, case_reference, live_keys, rel_err)

DEV = "cuda"
NAMES = ("o", "probs", "dq", "dk", "dv")


def _lens(values):
    return torch.tensor(values, dtype=torch.int32, device=DEV)


def run_len_p(q, k, v, g, Lq, Lk, dh, causal, key_len, period, mask=None, p=0.0, seed=0, ctr=None):
    """The two C entries on (B*L, H*dh) device tensors; key_len None: the unmasked ast_attn_fwd_p / ast_attn_bwd_p instead."""
    nb, d = q.shape[0] // Lq, H * dh
    o, dq = torch.empty_like(q), torch.empty_like(q)
    dk, dv = torch.empty_like(k), torch.empty_like(v)
    probs = torch.empty(nb, H, Lq, Lk, device=DEV)
    pm, pc = (None if mask is None else mask.data_ptr()), (None if ctr is None else ctr.data_ptr())
    a = (q.data_ptr(), k.data_ptr(), v.data_ptr())
    if key_len is None:
        ops.check(lib().ast_attn_fwd_p(*a, o.data_ptr(), probs.data_ptr(), nb, H, Lq, Lk, dh, d, d, d, int(causal), pm, p, seed, pc,
                                       ops.stream()), "ast_attn_fwd_p")
        ops.check(lib().ast_attn_bwd_p(g.data_ptr(), *a, probs.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), nb, H, Lq, Lk,
                                       dh, d, d, d, pm, p, seed, pc, ops.stream()), "ast_attn_bwd_p")
    else:
        ops.check(lib().ast_attn_fwd_len_p(*a, o.data_ptr(), probs.data_ptr(), nb, H, Lq, Lk, dh, d, d, d, int(causal),
                                           key_len.data_ptr(), period, pm, p, seed, pc, ops.stream()), "ast_attn_fwd_len_p")
        ops.check(lib().ast_attn_bwd_len_p(g.data_ptr(), *a, probs.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), nb, H, Lq,
                                           Lk, dh, d, d, d, key_len.data_ptr(), period, pm, p, seed, pc, ops.stream()),
                  "ast_attn_bwd_len_p")
    torch.cuda.synchronize()
    return dict(o=o, probs=probs, dq=dq, dk=dk, dv=dv)


def _case(idx, dropout):
    Lq, Lk, period, causal, dh, key_len = CASES[idx]
    q, k, v, g, mask = (t.to(DEV) for t in case_inputs(idx))
    return (q, k, v, g, Lq, Lk, dh, causal), key_len, period, (mask if dropout else None)


@pytest.mark.parametrize("idx", range(len(CASES)), ids=CASE_IDS)
@pytest.mark.parametrize("dropout", [False, True], ids=["p0", "p0.1"])
def test_core_against_float64(idx, dropout):
    """Measured worst errors (MI355X, of the tensor's scale): see DESIGN 7, "Masked attention in training"."""
    args, key_len, period, mask = _case(idx, dropout)
    Lk = args[5]
    got = run_len_p(*args, _lens(key_len), period, mask)
    ref = case_reference(idx, dropout)
    errs = {n: rel_err(got[n], ref[n]) for n in NAMES}
    print(f"masked core {CASE_IDS[idx]} dropout={dropout}: " + " ".join(f"{n}={e:.2e}" for n, e in errs.items()))
    for n, e in errs.items():
        assert e < GPU_TOL, (n, e)
    for b in range(B):
        dead = [j for j in range(Lk) if j not in live_keys(Lk, period, key_len[b])]
        assert int((got["probs"][b][:, :, dead] != 0).sum()) == 0, b           # dead is empty for the full-length clip
        for n in ("dk", "dv"):
            assert int((got[n].view(B, Lk, -1)[b, dead] != 0).sum()) == 0, (n, b)
    # an ignored mask cannot pass: the unmasked backward on the same padded inputs misses the reference (the CPU suite checks in
    # float64 that these seeds put it at least 10 tolerances away)
    un = run_len_p(*args, None, period, mask)
    for n in ("dq", "dk", "dv"):
        assert rel_err(un[n], ref[n]) > GPU_TOL, n


@pytest.mark.parametrize("idx", range(len(CASES)), ids=CASE_IDS)
def test_exact_properties_of_the_mask(idx):
    """With dropout on: NaN in every masked K and V row changes no output bit, device lengths out of range equal the clamped
    ones, and a second run is bit-identical."""
    args, key_len, period, mask = _case(idx, True)
    q, k, v, g, Lq, Lk, dh, causal = args
    got = run_len_p(*args, _lens(key_len), period, mask)
    again = run_len_p(*args, _lens(key_len), period, mask)
    kn, vn = k.clone().view(B, Lk, -1), v.clone().view(B, Lk, -1)
    for b in range(B):
        dead = [j for j in range(Lk) if j not in live_keys(Lk, period, key_len[b])]
        kn[b, dead] = float("nan")
        vn[b, dead] = float("nan")
    assert bool(torch.isnan(kn).any())
    nan = run_len_p(q, kn.view(B * Lk, -1), vn.view(B * Lk, -1), g, Lq, Lk, dh, causal, _lens(key_len), period, mask)
    clamped = run_len_p(*args, _lens([period, 1, 1]), period, mask)
    ranged = run_len_p(*args, _lens([period + 7, 0, -5]), period, mask)
    for n in NAMES:
        assert torch.equal(got[n], again[n]), n
        assert torch.equal(got[n], nan[n]), n
        assert torch.equal(clamped[n], ranged[n]), n


@pytest.mark.parametrize("Lq,Lk", [(8, 8), (33, 66)])
def test_full_lengths_equal_the_unmasked_kernels_bit_for_bit(Lq, Lk):
    """key_len = key_period = Lk, p = 0.1 drawn in the kernels from the same seed and counter."""
    dh, d = 64, H * 64
    gen = torch.Generator().manual_seed(97 + Lk)
    q, k, v, g = (torch.randn(n, d, generator=gen).to(DEV) for n in (B * Lq, B * Lk, B * Lk, B * Lq))
    ctr = torch.full((1,), 5, dtype=torch.int64, device=DEV)
    un = run_len_p(q, k, v, g, Lq, Lk, dh, False, None, Lk, None, P_DROP, 0x5EED + 7919, ctr)
    got = run_len_p(q, k, v, g, Lq, Lk, dh, False, _lens([Lk] * B), Lk, None, P_DROP, 0x5EED + 7919, ctr)
    nodrop = run_len_p(q, k, v, g, Lq, Lk, dh, False, _lens([Lk] * B), Lk, None, 0.0, 0, None)
    assert not torch.equal(got["o"], nodrop["o"])                  # the dropout was drawn
    for n in NAMES:
        assert torch.equal(got[n], un[n]), n


# ---- layers ------------------------------------------------------------------------------------------------------------------------
D, FF = 256, 1024
REL, ABS = 2e-3, 2e-4


def _close(got, ref, what):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    bound = torch.maximum(REL * torch.maximum(got.abs(), ref.abs()), torch.tensor(ABS, dtype=torch.float64))
    worst = float(((got - ref).abs() - bound).max())
    assert worst <= 0.0, (what, float((got - ref).abs().max()), float(ref.abs().max()))


def _seeded(make, seed, p=0.0):
    """make() -> modules, built and given random biases / LayerNorm parameters under one seed; every dropout probability set to p."""
    torch.manual_seed(seed)
    mods = make()
    for m in mods:
        for prm in m.parameters():
            with torch.no_grad():
                if prm.dim() == 1:
                    prm.add_(torch.randn_like(prm) * 0.1)
        for sub in m.modules():
            if isinstance(sub, nn.Dropout):
                sub.p = p
            if isinstance(sub, nn.MultiheadAttention):
                sub.dropout = p
    return [m.to(DEV) for m in mods]


def _grads(mods):
    return [prm.grad.detach().clone() for m in mods for prm in m.parameters()]


def _run(bank, mods, fn, inputs, w):
    """One forward and backward of loss = sum(out * w): returns out, the input gradients and the parameter gradients."""
    for m in mods:
        for prm in m.parameters():
            prm.grad = None
    leaves = [t.detach().contiguous().clone().requires_grad_(True) for t in inputs]
    bank.prepare(True)
    out = fn(*leaves)
    (out * w).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), [t.grad.detach().clone() for t in leaves], _grads(mods)


def _encoder(nlayers, seed=11, p=0.0):
    mods = _seeded(lambda: [nn.TransformerEncoderLayer(D, H, FF, dropout=0.1, batch_first=True) for _ in range(nlayers)], seed, p)
    config.set_compute_dtype(torch.float32)
    bank = AL.WeightBank()
    return bank, mods, [AL.EncoderLayer(bank, m) for m in mods]


def _padded(S, n, seed):
    """(B, S, D) with rows s >= n[b] zero, and the row mask (B, S, 1)."""
    gen = torch.Generator().manual_seed(seed)
    keep = (torch.arange(S)[None, :] < torch.tensor(n)[:, None]).float()[:, :, None]
    return (torch.randn(len(n), S, D, generator=gen) * keep).to(DEV), keep.to(DEV)


@pytest.mark.parametrize("fused", [True, False], ids=["fused_tokens", "plain"])
def test_encoder_stack_on_a_padded_batch_equals_each_clip_alone(fused, monkeypatch):
    monkeypatch.setattr(config, "fused_tokens", fused)
    n, S = [3, 1, 2], 3
    bank, mods, layers = _encoder(2)
    x, keep = _padded(S, n, 21)
    w = torch.randn(len(n), S, D, generator=torch.Generator().manual_seed(22)).to(DEV) * keep
    lengths = _lens(n)
    out, (dx,), grads = _run(bank, mods, lambda t: tokprog.run_encoder_stack(layers, t, True, lengths), [x], w)
    sums = None
    for b, nb in enumerate(n):
        ob, (dxb,), gb = _run(bank, mods, lambda t: tokprog.run_encoder_stack(layers, t, True), [x[b:b + 1, :nb]], w[b:b + 1, :nb])
        _close(out[b, :nb], ob[0], f"output of clip {b}")
        _close(dx[b, :nb], dxb[0], f"input gradient of clip {b}")
        assert int((dx[b, nb:] != 0).sum()) == 0, b                # padded rows: exactly 0
        sums = gb if sums is None else [a + c for a, c in zip(sums, gb)]
    for i, (a, c) in enumerate(zip(grads, sums)):
        _close(a, c, f"parameter gradient {i}")


@pytest.mark.parametrize("fused", [True, False], ids=["fused_tokens", "plain"])
@pytest.mark.parametrize("S,n", [(3, [3, 1, 2]), (9, [3, 1, 2]), (9, [9, 1, 2])], ids=["S3", "S9", "S9full"])
def test_decoder_layer_on_a_padded_batch_equals_each_clip_alone(S, n, fused, monkeypatch):
    """The memory is [content x S | class x S]; at S = 9 its 18 tokens reach csrc/attn.hip."""
    monkeypatch.setattr(config, "fused_tokens", fused)
    (mod,) = _seeded(lambda: [nn.TransformerDecoderLayer(D, H, FF, dropout=0.1, batch_first=True, norm_first=True)], 31)
    config.set_compute_dtype(torch.float32)
    bank = AL.WeightBank()
    layer = AL.DecoderLayer(bank, mod)
    x, keep = _padded(S, n, 41)
    ma, _ = _padded(S, n, 42)
    mb, _ = _padded(S, n, 43)
    mem = torch.cat([ma, mb], dim=1)
    w = torch.randn(len(n), S, D, generator=torch.Generator().manual_seed(44)).to(DEV) * keep
    lengths = _lens(n)
    out, (dx, dmem), grads = _run(bank, [mod], lambda t, m: layer(t, m, True, lengths), [x, mem], w)
    sums = None
    for b, nb in enumerate(n):
        mem_b = torch.cat([mem[b:b + 1, :nb], mem[b:b + 1, S:S + nb]], dim=1)
        ob, (dxb, dmb), gb = _run(bank, [mod], lambda t, m: layer(t, m, True), [x[b:b + 1, :nb], mem_b], w[b:b + 1, :nb])
        _close(out[b, :nb], ob[0], f"output of clip {b}")
        _close(dx[b, :nb], dxb[0], f"input gradient of clip {b}")
        _close(torch.cat([dmem[b, :nb], dmem[b, S:S + nb]]), dmb[0], f"memory gradient of clip {b}")
        sums = gb if sums is None else [a + c for a, c in zip(sums, gb)]
    for i, (a, c) in enumerate(zip(grads, sums)):
        _close(a, c, f"parameter gradient {i}")


def test_dropout_under_the_mask_repeats_bit_for_bit():
    """Dropout on (p = 0.1 everywhere), deterministic mode: two runs from the same _DropState give the same bits."""
    n, S = [3, 1, 2], 3
    with ast_amd.deterministic():
        bank, mods, layers = _encoder(1, p=0.1)
        x, keep = _padded(S, n, 51)
        w = torch.randn(len(n), S, D, generator=torch.Generator().manual_seed(52)).to(DEV) * keep
        lengths = _lens(n)
        fn = lambda t: layers[0](t, True, lengths)
        runs = []
        for _ in range(2):
            ops._DropState.calls = 7000
            runs.append(_run(bank, mods, fn, [x], w))
        ops._DropState.calls = 7100
        other = _run(bank, mods, fn, [x], w)
    (o1, (d1,), g1), (o2, (d2,), g2) = runs
    assert torch.equal(o1, o2) and torch.equal(d1, d2)
    for a, c in zip(g1, g2):
        assert torch.equal(a, c)
    assert not torch.equal(o1, other[0])                          # the dropout is on


def test_one_captured_graph_serves_every_mix_of_lengths():
    """EncoderLayer forward and backward with lengths in a torch.cuda.graph: replays with two key_len contents equal their eager
    runs bit for bit."""
    S, nclips = 3, 3
    with ast_amd.deterministic():
        bank, mods, layers = _encoder(1)
        x, _ = _padded(S, [S] * nclips, 61)
        w = torch.randn(nclips, S, D, generator=torch.Generator().manual_seed(62)).to(DEV)
        lengths = _lens([3, 1, 2])
        xs = x.clone().requires_grad_(True)

        def step():
            xs.grad = None
            out = layers[0](xs, True, lengths)
            (out * w).sum().backward()
            return out.detach(), xs.grad

        bank.prepare(True)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            g_out, g_dx = step()
        outs = []
        for mix in ([3, 1, 2], [2, 3, 1]):
            lengths.copy_(_lens(mix))
            graph.replay()
            torch.cuda.synchronize()
            r_out, r_dx = g_out.clone(), g_dx.clone()
            e_out, e_dx = step()
            torch.cuda.synchronize()
            assert torch.equal(r_out, e_out) and torch.equal(r_dx, e_dx), mix
            outs.append(r_out)
        assert not torch.equal(outs[0], outs[1])                  # the replay read the new lengths
