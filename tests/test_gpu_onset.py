"""Onsets and self-similarity on the device (ast_amd.onset_strength, onset_detect, onset_accuracy, recurrence_matrix,
self_similarity_distance; csrc/metrics.hip) and transfer_and_score(..., onsets=True, self_similarity=True).

Reference (tests/onset_ref.py): the float64 restatement of the chain.  Continuous outputs -- the envelope relative to the clip's
peak, the squared distances relative to the clip's largest -- must lie within 10 x the float32 floor, the same restatement in
float32 on the CPU against float64, computed where the test runs (about 3.6e-7 and 2.2e-6).  Discrete outputs -- onset masks, R,
onset_accuracy, self_similarity_distance -- must equal the restatement exactly; tests/test_onset_cpu.py shows that every decision
behind them lies 10 float32 errors from its threshold.  R of the silent clip and of the one-sample clips is decided by rounding
noise in any precision (onset_ref.ranked_clips); for those, R must equal the neighbour rule applied to the device's own distances,
which every clip is checked for as well.  The figures reached on the MI355X are in DESIGN 7, "Onsets and self-similarity"."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import ast_amd
    from ast_amd import config
    from ast_amd import metrics as M
    from ast_amd.infer import StyleTransferSession

import onset_ref as F

DEV = "cuda"
MODES = ["constant", "reflect"]


def i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def waves(fill=None, pad_mode="constant"):
    """the fixture on the device; fill: that value behind every clip's end"""
    a, g = (t.to(DEV).clone() for t in F.fixture_waves())
    if fill is not None:
        for b in range(F.B):
            a[b, F.COUNTS[pad_mode][b]:] = fill
            g[b, F.N_GENERATED[pad_mode][b]:] = fill
    return a, g


def f32(v):
    return torch.tensor(v, dtype=torch.float64).float()


@pytest.mark.parametrize("pad_mode", MODES)
def test_outputs_match_the_float64_restatement(pad_mode):
    a, g = waves()
    counts = dict(orig=F.COUNTS[pad_mode], gen=F.N_GENERATED[pad_mode])
    ref, bound, floor = F.references(pad_mode), F.bounds(pad_mode), F.f32_floor(pad_mode)
    e_env, e_d2 = [], []
    for which, w in (("orig", a), ("gen", g)):
        ns = i32(counts[which])
        env, mask = M.onset_strength(w, ns, pad_mode).cpu(), M.onset_detect(w, ns, pad_mode).cpu()
        R, d2 = (t.cpu() for t in M.recurrence_debug(w, ns, pad_mode))
        assert torch.equal(R, M.recurrence_matrix(w, ns, pad_mode).cpu())
        T_max = 1 + w.shape[1] // F.HOP
        assert env.shape == mask.shape == (F.B, T_max) and env.dtype == torch.float32 and mask.dtype == torch.int32
        assert R.shape == d2.shape == (F.B, 20, 20) and R.dtype == torch.int32
        for b in range(F.B):
            r = ref[which][b]
            T = len(r["env"])
            assert T == F.n_frames(counts[which][b])
            e_env.append(F.env_error(env[b, :T].numpy(), r["env"]))
            assert float(env[b, T:].abs().max() if T < T_max else 0) == 0.0 and float(env[b, :min(T, 3)].abs().max()) == 0.0
            assert np.array_equal(mask[b, :T].numpy().astype(bool), r["mask"]), (which, b, mask[b].tolist())          # exactly
            assert int(mask[b, T:].sum()) == 0 and set(mask[b].tolist()) <= {0, 1}
            e_d2.append(F.d2_error(d2[b].numpy(), r["d2"]))
            Rb = R[b].numpy()
            assert np.array_equal(Rb, F.neighbour_rule(d2[b].numpy())), (which, b)     # the rule on the device's own distances: every clip
            assert int(Rb.sum(axis=0).max()) <= F.K and int(np.trace(Rb)) == 0 and set(Rb.ravel().tolist()) <= {0, 1}
            if (which, b) in F.ranked_clips(pad_mode):
                assert np.array_equal(Rb, r["R"]), (which, b)                           # exactly
    print(f"{pad_mode}: envelope {max(e_env):.3g} (floor {floor['env']:.3g}, bound {bound['env']:.3g}), squared distances {max(e_d2):.3g} "
          f"(floor {floor['d2']:.3g}, bound {bound['d2']:.3g})")
    assert max(e_env) <= bound["env"], e_env
    assert max(e_d2) <= bound["d2"], e_d2
    na, ng = i32(counts["orig"]), i32(counts["gen"])
    acc = M.onset_accuracy(a, g, na, ng, pad_mode).cpu()
    ssd = M.self_similarity_distance(a, g, na, ng, pad_mode).cpu()
    print(f"{pad_mode}: onset_accuracy {acc.tolist()}, self_similarity_distance {ssd.tolist()}")
    assert torch.equal(acc, f32(ref["acc"])) and 0 < float(acc[0]) < 1                  # exactly
    Ra, Rg = M.recurrence_matrix(a, na, pad_mode), M.recurrence_matrix(g, ng, pad_mode)
    assert torch.equal(ssd, ((Ra - Rg).abs().sum(dim=(1, 2)).double() / 400).float().cpu())
    for b in range(F.B):
        if ("orig", b) in F.ranked_clips(pad_mode) and ("gen", b) in F.ranked_clips(pad_mode):
            assert float(ssd[b]) == float(f32(ref["ssd"])[b]), b                        # exactly
    assert sum(("orig", b) in F.ranked_clips(pad_mode) and ("gen", b) in F.ranked_clips(pad_mode) for b in range(F.B)) >= 2


@pytest.mark.parametrize("pad_mode", MODES)
def test_known_answers(pad_mode):
    a, g = waves()
    na, ng = i32(F.COUNTS[pad_mode]), i32(F.N_GENERATED[pad_mode])
    assert M.onset_accuracy(a, a, na, na, pad_mode).tolist() == [1.0] * F.B            # exactly
    assert M.onset_accuracy(g, g.clone(), None, None, pad_mode).tolist() == [1.0] * F.B
    assert M.self_similarity_distance(a, a, na, na, pad_mode).tolist() == [0.0] * F.B
    assert M.self_similarity_distance(g, g.clone(), None, None, pad_mode).tolist() == [0.0] * F.B
    zero = torch.zeros(F.B, 5000, device=DEV)
    assert M.onset_accuracy(zero, zero, None, None, pad_mode).tolist() == [1.0] * F.B   # silence against silence
    assert int(M.onset_detect(zero, None, pad_mode).sum()) == 0 and float(M.onset_strength(zero, None, pad_mode).abs().max()) == 0.0
    burst = g[2:3, :5000].repeat(F.B, 1).contiguous()
    assert int(M.onset_detect(burst, None, pad_mode).sum()) >= F.B
    assert M.onset_accuracy(zero, burst, None, None, pad_mode).tolist() == [0.0] * F.B  # silence against bursts, either way round
    assert M.onset_accuracy(burst, zero, None, None, pad_mode).tolist() == [0.0] * F.B
    assert float(M.onset_accuracy(a, g, na, ng, pad_mode)[2]) == 0.0                    # the fixture's silent row
    # the short clips (T <= 3) have no onsets, whatever they hold
    assert int(M.onset_detect(a, na, pad_mode)[3].sum()) == 0 and int(M.onset_detect(g, ng, pad_mode)[3].sum()) == 0
    assert float(M.onset_accuracy(a, g, na, ng, pad_mode)[3]) == 1.0
    # silence: c_0 = -100 sqrt(128), the other rows are rounding noise, so every distance to row 0 is the largest of its column;
    # R holds what the rule leaves of the device's own distances -- exact zeros among them are dropped
    R, d2 = (t.cpu().numpy() for t in M.recurrence_debug(zero, None, pad_mode))
    for b in range(F.B):
        assert np.array_equal(R[b], F.neighbour_rule(d2[b])) and int(R[b].sum(axis=0).max()) <= F.K and int(np.trace(R[b])) == 0
        assert np.all(R[b][d2[b] == 0] == 0)
        sub = d2[b][1:, 1:]
        assert float(sub.max()) <= 1e-8 * float(d2[b].max()) and float(d2[b][0, 1:].min()) > 0.99 * float(d2[b].max())
        assert np.array_equal(R[b], R[0]) and np.array_equal(d2[b], d2[0])


@pytest.mark.parametrize("pad_mode", MODES)
def test_ragged_contract(pad_mode):
    a, g = waves()
    ca, cg, lo = F.COUNTS[pad_mode], F.N_GENERATED[pad_mode], (1025 if pad_mode == "reflect" else 1)
    na, ng = i32(ca), i32(cg)

    def singles(w, ns):
        return (M.onset_strength(w, ns, pad_mode), M.onset_detect(w, ns, pad_mode)) + M.recurrence_debug(w, ns, pad_mode)

    def pairs(x, y, nx, ny):
        return M.onset_accuracy(x, y, nx, ny, pad_mode), M.self_similarity_distance(x, y, nx, ny, pad_mode)

    def same(p, q):
        return all(torch.equal(s, t) for s, t in zip(p, q))

    one, two = singles(a, na), pairs(a, g, na, ng)
    for b in range(F.B):
        # row b of the padded batch is the clip alone at B = 1, bit for bit, and exactly 0 behind its frames
        xa, xg = a[b:b + 1, :ca[b]].contiguous(), g[b:b + 1, :cg[b]].contiguous()
        T = F.n_frames(ca[b])
        alone = singles(xa, None)
        assert torch.equal(alone[0][0], one[0][b, :T]) and torch.equal(alone[1][0], one[1][b, :T]), b
        assert torch.equal(alone[2][0], one[2][b]) and torch.equal(alone[3][0], one[3][b]), b
        assert int((one[0][b, T:] != 0).sum()) == 0 and int((one[1][b, T:] != 0).sum()) == 0 and bool(torch.isfinite(one[0][b]).all()), b
        assert same(pairs(xa, xg, None, None), [t[b:b + 1] for t in two]), b
    # NaN behind every clip's end changes nothing
    an, gn = waves(fill=float("nan"), pad_mode=pad_mode)
    assert same(singles(an, na), one) and same(pairs(an, gn, na, ng), two)
    # device counts outside the range equal the clamped ones
    wild, clamped = i32([0, -5, F.N_ORIG + 9, ca[3]]), i32([lo, lo, F.N_ORIG, ca[3]])
    assert same(singles(a, wild), singles(a, clamped))
    assert same(pairs(a, g, wild, ng), pairs(a, g, clamped, ng)) and same(pairs(g, a, ng, wild), pairs(g, a, ng, clamped))
    # no counts: the rows are full
    full_a, full_g = i32([F.N_ORIG] * F.B), i32([F.N_GEN] * F.B)
    assert same(singles(a, None), singles(a, full_a))
    assert same(pairs(a, g, None, ng), pairs(a, g, full_a, ng)) and same(pairs(a, g, na, None), pairs(a, g, na, full_g))
    # repeats are bitwise equal; rows of different widths in a pair (the fixture's are; narrower still changes nothing)
    assert same(singles(a, na), one) and same(pairs(a, g, na, ng), two)
    assert a.shape[1] != g.shape[1] and same(pairs(a, g[:, :10400].contiguous(), na, ng), two)


def test_wrappers_refuse_bad_arguments_on_the_device():
    ok = torch.zeros(2, 3000, device=DEV)
    for fn in (M.onset_strength, M.onset_detect, M.recurrence_matrix):
        with pytest.raises(ValueError):
            fn(ok, pad_mode="edge")
        with pytest.raises(ValueError, match="1025"):
            fn(torch.zeros(2, 1024, device=DEV), pad_mode="reflect")
        with pytest.raises(ValueError, match="n_samples"):
            fn(ok, torch.zeros(2, dtype=torch.int64, device=DEV))
    for fn in (M.onset_accuracy, M.self_similarity_distance):
        with pytest.raises(ValueError, match="1025"):
            fn(ok, torch.zeros(2, 1024, device=DEV), pad_mode="reflect")
        with pytest.raises(ValueError):
            fn(ok, torch.zeros(3, 3000, device=DEV))
    assert M.onset_strength(ok).shape == (2, 6) and M.onset_detect(ok).shape == (2, 6) and M.recurrence_matrix(ok).shape == (2, 20, 20)


# ---- transfer_and_score(..., onsets=True, self_similarity=True) ------------------------------------------------------------------------
def test_transfer_and_score_with_onsets_and_self_similarity():
    """In bf16, where two runs of the session agree bit for bit (test_gpu_ragged_wave: the f32 session has run-to-run noise, so
    'bit-equal to the call without the flags' can only be asked of bf16)."""
    from test_gpu_ragged_wave import _seeded, padded_batch
    from test_ragged_wave_cpu import NS
    from oracle import seeded_params as sp
    config.set_compute_dtype(torch.bfloat16)
    try:
        _session_check(_seeded, padded_batch, NS, sp)
    finally:
        config.set_compute_dtype(torch.float32)


def _session_check(_seeded, padded_batch, NS, sp):
    enc, dec = _seeded("content", ast_amd.ContentEncoder), _seeded("decoder", ast_amd.Decoder)
    cls = sp.seeded_normal((2, 256), 7710).to(DEV)
    eager, graph = StyleTransferSession(enc, dec, use_graph=False), StyleTransferSession(enc, dec, use_graph=True)
    new = ["onset_accuracy", "self_similarity_distance"]
    for order in ([0, 2], [2, 0]):                                    # 85 760 and 36 708 samples, then swapped
        wav, n = padded_batch(order)
        ref_w, ref_n = padded_batch(order[::-1])
        assert sorted(n.tolist()) == [36708, 85760] and n.tolist() == [NS[b] for b in order]
        for sess in (eager, graph):
            plain = sess.transfer_and_score(wav, cls, n_samples=n, reference=ref_w, n_reference=ref_n)
            want = tuple(t.clone() for t in plain[:3]) + ({k: v.clone() for k, v in plain[3].items()},)
            assert sorted(want[3]) == ["instrumentation_similarity", "mse_spectrogram"]
            keys_before = set(sess._graphs)
            res = sess.transfer_and_score(wav, cls, n_samples=n, reference=ref_w, n_reference=ref_n, onsets=True, self_similarity=True)
            assert len(res) == 4 and sorted(res[3]) == sorted(list(want[3]) + new)
            for got, exp in zip(res[:3], want[:3]):                   # every other output: bit-equal to the call without the flags
                assert torch.equal(got, exp)
            for k in want[3]:
                assert torch.equal(res[3][k], want[3][k]), k
            acc, ssd = res[3]["onset_accuracy"], res[3]["self_similarity_distance"]
            print(f"transfer_and_score(onsets, self_similarity), {'graph' if sess is graph else 'eager'}, order {order}: "
                  f"onset_accuracy {acc.tolist()}, self_similarity_distance {ssd.tolist()}")
            assert acc.shape == ssd.shape == (2,) and bool(((acc >= 0) & (acc <= 1)).all()) and bool(((ssd >= 0) & (ssd <= 1)).all())
            assert torch.equal(acc, M.onset_accuracy(wav, res[0], n, res[2]))                         # the stand-alone functions, bit for bit
            assert torch.equal(ssd, M.self_similarity_distance(res[0], ref_w, res[2], ref_n))
            with pytest.raises(ValueError, match="reference"):
                sess.transfer_and_score(wav, cls, n_samples=n, self_similarity=True)
            only = sess.transfer_and_score(wav, cls, n_samples=n, onsets=True)                         # needs no reference
            assert sorted(only[3]) == ["mse_spectrogram", "onset_accuracy"] and torch.equal(only[3]["onset_accuracy"], acc)
            if sess is graph:                                         # the default call keeps its key; the flags add their own words
                added = set(sess._graphs) - keys_before
                assert keys_before <= set(sess._graphs) and all("onsets" in k for k in added)
                assert not any("onsets" in k or "self_similarity" in k for k in keys_before if order == [0, 2])
    # plain, both flags, onsets alone: the swapped batch replayed all three
    assert len(graph._graphs) == 3
    assert sum("self_similarity" in k for k in graph._graphs) == 1 and sum("onsets" in k for k in graph._graphs) == 2
