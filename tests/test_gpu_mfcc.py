"""MFCC on the device (ast_amd.mfcc, ast_amd.mfcc_distance, csrc/metrics.hip) and transfer_and_score(..., mfcc=True).

Reference and bounds (tests/mfcc_ref.py): the float64 restatement of librosa.feature.mfcc's documented formula chain.  The
tolerance is the project's rule, 10 x the float32 floor -- the same restatement in float32 on the CPU against its float64 form,
maximum over the fixture's rows, both batches and the two settings (13 coefficients at hop 256, 20 at hop 512).  Error measures:
coefficients, the largest absolute error over a clip relative to the clip's peak |coefficient|; distances, the absolute error
relative to the pair's peak |coefficient| (mfcc_ref.dist_error says why).  The floors are computed where the test runs
(about 1.4e-6 for coefficients, 3.4e-7 / 8.8e-8 for constant / reflect distances); the figures the kernels reached on the MI355X
are in DESIGN 7, "MFCC"."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import ast_amd
    from ast_amd import _lib, config
    from ast_amd import metrics as M
    from ast_amd.infer import StyleTransferSession

import mfcc_ref as F

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


def test_fixture_reaches_every_run_and_tile_case():
    run = _lib.lib().ast_mfcc_run_frames()
    for hop in (256, 512):
        frames = sorted({1 + n // hop for pm in MODES for n in F.COUNTS[pm] + F.N_GENERATED[pm]})
        assert any(T < run for T in frames) and any(T > run and T % run for T in frames), (hop, frames)
        assert any(T > 32 and T % 32 for T in frames), (hop, frames)           # more than one tile of the second pass, the last one ragged
    assert any((1 + n // 512) % run == 0 for n in F.COUNTS["constant"])        # a clip of exactly whole runs


@pytest.mark.parametrize("n_mfcc,hop", F.SETTINGS)
@pytest.mark.parametrize("pad_mode", MODES)
def test_mfcc_matches_the_float64_restatement(pad_mode, n_mfcc, hop):
    a, g = waves()
    na, ng = i32(F.COUNTS[pad_mode]), i32(F.N_GENERATED[pad_mode])
    ref, bound, floor = F.references(pad_mode, n_mfcc, hop), F.bounds(pad_mode), F.f32_floor(pad_mode)
    ma, mg = M.mfcc(a, na, n_mfcc, hop, pad_mode).cpu(), M.mfcc(g, ng, n_mfcc, hop, pad_mode).cpu()
    dist = M.mfcc_distance(g, a, ng, na, n_mfcc, hop, pad_mode).cpu()
    assert ma.shape == mg.shape == (F.B, n_mfcc, 1 + F.N_MAX // hop) and ma.dtype == torch.float32 and dist.shape == (F.B,)
    e_coef, e_dist = [], []
    for b in range(F.B):
        for got, which in ((ma, "orig"), (mg, "gen")):
            T = ref[which][b].shape[1]
            e_coef.append(F.coef_error(got[b, :, :T], ref, which, b))
            assert float(got[b, :, T:].abs().max()) == 0.0 if T < got.shape[2] else True, (which, b)
        e_dist.append(F.dist_error(dist[b], ref, b))
    print(f"{pad_mode} n_mfcc {n_mfcc} hop {hop}: coefficients {max(e_coef):.3g} (floor {floor['coef']:.3g}, bound {bound['coef']:.3g}), "
          f"distance {max(e_dist):.3g} (floor {floor['dist']:.3g}, bound {bound['dist']:.3g}); per row {['%.2g' % e for e in e_dist]}; "
          f"distances {dist.tolist()}")
    assert max(e_coef) <= bound["coef"], e_coef
    assert max(e_dist) <= bound["dist"], e_dist


@pytest.mark.parametrize("pad_mode", MODES)
def test_known_answers(pad_mode):
    a, _ = waves()
    na = i32(F.COUNTS[pad_mode])
    bound = F.bounds(pad_mode)
    for n_mfcc, hop in F.SETTINGS:
        assert M.mfcc_distance(a, a, na, na, n_mfcc, hop, pad_mode).tolist() == [0.0] * F.B            # exactly
        assert M.mfcc_distance(a, a.clone(), None, None, n_mfcc, hop, pad_mode).tolist() == [0.0] * F.B
    # row 0 touches neither clamp: doubling the clip adds 20 log10(2) to every mel value, all of it in coefficient 0
    want = 20 * math.log10(2) * math.sqrt(128)
    got = float(M.mfcc_distance(a[:1], 2 * a[:1], pad_mode=pad_mode)[0])
    peak = F.references(pad_mode, 13, 256)["peak_orig"][0]
    print(f"{pad_mode}: mfcc_distance(a, 2a) = {got:.6f}, wanted {want:.6f}: {abs(got - want) / peak:.3g} of the peak (bound {bound['dist']:.3g})")
    assert abs(want - 68.11531) < 1e-5 and abs(got - want) / peak <= bound["dist"]
    # silence: every mel value sits on the 1e-10 floor, -100 dB, above the clip's maximum - 80
    zero = torch.zeros(2, 5000, device=DEV)
    c0 = -100 * math.sqrt(128)
    for n_mfcc, hop in F.SETTINGS:
        m = M.mfcc(zero, None, n_mfcc, hop, pad_mode).cpu().double()
        assert m.shape == (2, n_mfcc, 1 + 5000 // hop)
        e0, e1 = float((m[:, 0] - c0).abs().max()) / -c0, float(m[:, 1:].abs().max()) / -c0
        print(f"{pad_mode} n_mfcc {n_mfcc} hop {hop}: silence c_0 off by {e0:.3g}, the others by {e1:.3g} of |c_0| (bound {bound['coef']:.3g})")
        assert abs(c0 + 1131.3708) < 1e-4 and e0 <= bound["coef"] and e1 <= bound["coef"]
        assert M.mfcc_distance(zero, zero, None, None, n_mfcc, hop, pad_mode).tolist() == [0.0, 0.0]


@pytest.mark.parametrize("pad_mode", MODES)
def test_ragged_contract(pad_mode):
    a, g = waves()
    ca, cg, lo = F.COUNTS[pad_mode], F.N_GENERATED[pad_mode], (1025 if pad_mode == "reflect" else 1)
    na, ng = i32(ca), i32(cg)
    for n_mfcc, hop in F.SETTINGS:
        m, d = M.mfcc(a, na, n_mfcc, hop, pad_mode), M.mfcc_distance(g, a, ng, na, n_mfcc, hop, pad_mode)
        for b in range(F.B):
            # row b of the padded batch is the clip alone at B = 1, bit for bit, and exactly 0 behind its frames
            xa, xg = a[b:b + 1, :ca[b]].contiguous(), g[b:b + 1, :cg[b]].contiguous()
            T = 1 + ca[b] // hop
            assert torch.equal(M.mfcc(xa, None, n_mfcc, hop, pad_mode)[0], m[b, :, :T]), b
            assert int((m[b, :, T:] != 0).sum()) == 0 and bool(torch.isfinite(m[b]).all()), b
            assert torch.equal(M.mfcc_distance(xg, xa, None, None, n_mfcc, hop, pad_mode), d[b:b + 1]), b
        # NaN behind every clip's end changes nothing
        an, gn = waves(fill=float("nan"), pad_mode=pad_mode)
        assert torch.equal(M.mfcc(an, na, n_mfcc, hop, pad_mode), m) and torch.equal(M.mfcc_distance(gn, an, ng, na, n_mfcc, hop, pad_mode), d)
        # device counts outside the range equal the clamped ones
        wild, clamped = i32([0, -5, F.N_MAX + 9, ca[3]]), i32([lo, lo, F.N_MAX, ca[3]])
        assert torch.equal(M.mfcc(a, wild, n_mfcc, hop, pad_mode), M.mfcc(a, clamped, n_mfcc, hop, pad_mode))
        assert torch.equal(M.mfcc_distance(g, a, ng, wild, n_mfcc, hop, pad_mode), M.mfcc_distance(g, a, ng, clamped, n_mfcc, hop, pad_mode))
        assert torch.equal(M.mfcc_distance(a, g, wild, ng, n_mfcc, hop, pad_mode), M.mfcc_distance(a, g, clamped, ng, n_mfcc, hop, pad_mode))
        # no counts: the rows are full
        full = i32([F.N_MAX] * F.B)
        assert torch.equal(M.mfcc(a, None, n_mfcc, hop, pad_mode), M.mfcc(a, full, n_mfcc, hop, pad_mode))
        assert torch.equal(M.mfcc_distance(g, a, None, na, n_mfcc, hop, pad_mode), M.mfcc_distance(g, a, full, na, n_mfcc, hop, pad_mode))
        # repeats are bitwise equal; rows of different widths
        assert torch.equal(M.mfcc(a, na, n_mfcc, hop, pad_mode), m) and torch.equal(M.mfcc_distance(g, a, ng, na, n_mfcc, hop, pad_mode), d)
        assert torch.equal(M.mfcc_distance(g[:, :30000].contiguous(), a, ng, na, n_mfcc, hop, pad_mode), d)


def test_wrappers_refuse_bad_arguments_on_the_device():
    ok = torch.zeros(2, 3000, device=DEV)
    for kw in (dict(n_mfcc=0), dict(n_mfcc=129), dict(n_mfcc=13.0), dict(hop_length=128), dict(hop_length=1024), dict(pad_mode="edge")):
        with pytest.raises(ValueError):
            M.mfcc(ok, **kw)
        with pytest.raises(ValueError):
            M.mfcc_distance(ok, ok, **kw)
    with pytest.raises(ValueError, match="1025"):
        M.mfcc_distance(ok, torch.zeros(2, 1024, device=DEV), pad_mode="reflect")
    assert M.mfcc(ok, n_mfcc=128).shape == (2, 128, 6) and M.mfcc(ok, n_mfcc=1, hop_length=256).shape == (2, 1, 12)


# ---- transfer_and_score(..., mfcc=True) ------------------------------------------------------------------------------------------------
def test_transfer_and_score_with_mfcc():
    """In bf16, where two runs of the session agree bit for bit (test_gpu_ragged_wave: the f32 session has run-to-run noise of
    5.3e-7, so 'bit-equal to mfcc=False' can only be asked of bf16)."""
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
    for order in ([0, 2], [2, 0]):                                    # 85 760 and 36 708 samples, then swapped
        wav, n = padded_batch(order)
        ref_w, ref_n = padded_batch(order[::-1])
        assert sorted(n.tolist()) == [36708, 85760] and n.tolist() == [NS[b] for b in order]
        for sess in (eager, graph):
            plain = sess.transfer_and_score(wav, cls, n_samples=n, reference=ref_w, n_reference=ref_n)
            want = tuple(t.clone() for t in plain[:3]) + ({k: v.clone() for k, v in plain[3].items()},)
            assert sorted(want[3]) == ["instrumentation_similarity", "mse_spectrogram"]
            res = sess.transfer_and_score(wav, cls, n_samples=n, reference=ref_w, n_reference=ref_n, mfcc=True)
            assert len(res) == 4 and sorted(res[3]) == ["instrumentation_similarity", "mfcc_distance", "mse_spectrogram"]
            for got, exp in zip(res[:3], want[:3]):                   # the first three outputs and the old scores: bit-equal to mfcc=False
                assert torch.equal(got, exp)
            for k in want[3]:
                assert torch.equal(res[3][k], want[3][k]), k
            d = res[3]["mfcc_distance"]
            print(f"transfer_and_score(mfcc=True), {'graph' if sess is graph else 'eager'}, order {order}: mfcc_distance {d.tolist()}")
            assert d.shape == (2,) and bool(torch.isfinite(d).all()) and bool((d > 0).all())
            assert torch.equal(d, M.mfcc_distance(res[0], ref_w, res[2], ref_n))                     # the stand-alone function, bit for bit
            with pytest.raises(ValueError, match="reference"):
                sess.transfer_and_score(wav, cls, n_samples=n, mfcc=True)
    assert len(graph._graphs) == 2                                    # with and without mfcc: the swapped batch replayed both
