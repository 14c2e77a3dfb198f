"""Chroma and pitch metrics on the device (ast_amd.estimate_tuning, chroma_stft, chroma_distance, chroma_similarity, pitch_mean,
pitch_correlation; csrc/chroma.hip) and transfer_and_score(..., chroma=True).

Reference and bounds (tests/chroma_ref.py): the float64 restatement of librosa's documented chain.  The tolerance is the project's
rule, 10 x the float32 floor -- the same restatement in float32 on the CPU against its float64 form, computed where the test runs,
maximum over the fixture's rows and both batches.  Error measures: chroma and mean pitch, the largest absolute error over a clip
relative to the clip's peak value; the median, relative; the three scores, absolute (they are of order 1).  The tuning pass is
compared through its debug output: counts and the histogram to within the allowance A = max(4, 10 x the twin's L1 histogram
difference), the tuning itself exactly (tests/test_chroma_cpu.py checks that the fixture's histograms have a winner that A
cannot unseat).  The figures the kernels reached on the MI355X are in DESIGN 7, "Chroma and pitch"."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import ast_amd
    from ast_amd import _lib, config
    from ast_amd import metrics as M
    from ast_amd.infer import StyleTransferSession

import chroma_ref as F

DEV = "cuda"
MODES = ["constant", "reflect"]
SETTINGS = [F.WIDE, F.NARROW]


def i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def waves(fill=None):
    """the fixture on the device; fill: that value behind every clip's end"""
    a, g = (t.to(DEV).clone() for t in F.fixture_waves())
    if fill is not None:
        for b in range(F.B):
            a[b, F.COUNTS[b]:] = fill
            g[b, F.N_GENERATED[b]:] = fill
    return a, g


def batches():
    a, g = waves()
    return ((0, a, F.COUNTS), (1, g, F.N_GENERATED))


@pytest.mark.parametrize("pad_mode", MODES)
def test_chroma_and_pitch_with_supplied_tuning(pad_mode):
    ref, bound, floor = F.references(pad_mode), F.bounds(pad_mode), F.f32_floor(pad_mode)
    e_chroma, e_pitch = [], []
    for j, x, counts in batches():
        p = M.pitch_mean(x, i32(counts), pad_mode).cpu()
        assert p.shape == (F.B, 1 + F.N_MAX // 512) and p.dtype == torch.float32
        for b in range(F.B):
            T = len(ref["pitch"][b][j])
            e_pitch.append(F.peak_error(p[b, :T].numpy(), ref["pitch"][b][j]))
            assert not p[b, T:].any(), (j, b)
        for s in SETTINGS:
            tuning = torch.tensor([ref["info", s][b][j]["tuning"] for b in range(F.B)], dtype=torch.float32, device=DEV)
            c = M.chroma_stft(x, i32(counts), s[0], s[1], pad_mode, tuning=tuning).cpu()
            assert c.shape == (F.B, 12, 1 + F.N_MAX // s[1]) and c.dtype == torch.float32
            for b in range(F.B):
                T = ref["chroma", s][b][j].shape[1]
                e_chroma.append(F.peak_error(c[b, :, :T].numpy(), ref["chroma", s][b][j]))
                assert not c[b, :, T:].any(), (s, j, b)
    print(f"{pad_mode}: chroma {max(e_chroma):.3g} (floor {floor['chroma']:.3g}, bound {bound['chroma']:.3g}), "
          f"mean pitch {max(e_pitch):.3g} (floor {floor['pitch']:.3g}, bound {bound['pitch']:.3g})")
    assert max(e_chroma) <= bound["chroma"], e_chroma
    assert max(e_pitch) <= bound["pitch"], e_pitch


@pytest.mark.parametrize("pad_mode", MODES)
def test_tuning_pass(pad_mode):
    ref, bound, floor = F.references(pad_mode), F.bounds(pad_mode), F.f32_floor(pad_mode)
    e_thr, worst = [], [0, 0, 0]
    for s in SETTINGS:
        for j, x, counts in batches():
            tuning, n, kept, thr, hist = (t.cpu() for t in M.tuning_debug(x, i32(counts), s[0], s[1], pad_mode))
            assert torch.equal(tuning, M.estimate_tuning(x, i32(counts), s[0], s[1], pad_mode).cpu())
            for b in range(F.B):
                want, A = ref["info", s][b][j], F.allowance(pad_mode, s, b, j)
                l1 = int(np.abs(hist[b].numpy().astype(np.int64) - want["hist"]).sum())
                worst = [max(worst[0], abs(int(n[b]) - want["n"])), max(worst[1], abs(int(kept[b]) - want["kept"])), max(worst[2], l1)]
                assert abs(int(n[b]) - want["n"]) <= A and abs(int(kept[b]) - want["kept"]) <= A and l1 <= A, (s, j, b, int(n[b]), want["n"], l1, A)
                assert int(hist[b].sum()) == int(kept[b])
                e_thr.append(abs(float(thr[b]) - want["thr"]) / want["thr"])
                assert float(tuning[b]) == float(np.float32(want["tuning"])), (s, j, b, float(tuning[b]), want["tuning"])
    print(f"{pad_mode}: peaks off by at most {worst[0]}, kept by {worst[1]}, histogram L1 {worst[2]} (allowance 4); median {max(e_thr):.3g} "
          f"(floor {floor['thr']:.3g}, bound {bound['thr']:.3g})")
    assert max(e_thr) <= bound["thr"], e_thr


@pytest.mark.parametrize("pad_mode", MODES)
def test_scores_match_the_float64_restatement(pad_mode):
    a, g = waves()
    na, ng = i32(F.COUNTS), i32(F.N_GENERATED)
    ref, bound, floor = F.references(pad_mode), F.bounds(pad_mode), F.f32_floor(pad_mode)
    got = dict(dist=M.chroma_distance(a, g, na, ng, pad_mode), sim=M.chroma_similarity(g, a, ng, na, pad_mode),
               corr=M.pitch_correlation(a, g, na, ng, pad_mode))
    for k, v in got.items():
        assert v.shape == (F.B,) and v.dtype == torch.float32
        err = [abs(float(v[b]) - ref[k][b]) for b in range(F.B)]
        print(f"{pad_mode} {k}: {max(err):.3g} (floor {floor[k]:.3g}, bound {bound[k]:.3g}); per row {['%.2g' % e for e in err]}; values {v.tolist()}")
    for k, v in got.items():
        assert max(abs(float(v[b]) - ref[k][b]) for b in range(F.B)) <= bound[k], k


@pytest.mark.parametrize("pad_mode", MODES)
def test_known_answers(pad_mode):
    a, _ = waves()
    na = i32(F.COUNTS)
    bound = F.bounds(pad_mode)
    assert M.chroma_distance(a, a, na, na, pad_mode).tolist() == [0.0] * F.B            # exactly
    assert M.chroma_distance(a, a.clone(), None, None, pad_mode).tolist() == [0.0] * F.B
    sim, corr = M.chroma_similarity(a, a, na, na, pad_mode).cpu(), M.pitch_correlation(a, a, na, na, pad_mode).cpu()
    print(f"{pad_mode}: chroma_similarity(a, a) - 1 = {(sim - 1).tolist()}, pitch_correlation(a, a) - 1 = {(corr - 1).tolist()}")
    assert float((sim - 1).abs().max()) <= bound["sim"] and float((corr - 1).abs().max()) <= bound["corr"]
    zero = torch.zeros(2, 5000, device=DEV)
    for n_fft, hop in SETTINGS:
        assert M.estimate_tuning(zero, None, n_fft, hop, pad_mode).tolist() == [0.0, 0.0]
        c = M.chroma_stft(zero, None, n_fft, hop, pad_mode)
        assert c.shape == (2, 12, 1 + 5000 // hop) and not c.any()
    assert not M.pitch_mean(zero, None, pad_mode).any()
    assert M.chroma_similarity(zero, zero, None, None, pad_mode).tolist() == [0.0, 0.0]
    assert M.chroma_similarity(zero, a[:2, :5000].contiguous(), None, None, pad_mode).tolist() == [0.0, 0.0]
    assert M.pitch_correlation(zero, zero, None, None, pad_mode).tolist() == [0.0, 0.0]
    assert M.chroma_distance(zero, zero, None, None, pad_mode).tolist() == [0.0, 0.0]
    # fewer than 2 frames: Pearson's r does not exist
    if pad_mode == "constant":
        assert M.pitch_correlation(a, a, i32([300] * F.B), na).tolist() == [0.0] * F.B
        assert M.chroma_similarity(a, a, i32([200] * F.B), na).tolist() == [0.0] * F.B


@pytest.mark.parametrize("pad_mode", MODES)
def test_ragged_contract(pad_mode):
    a, g = waves()
    ca, cg = F.COUNTS, F.N_GENERATED
    na, ng = i32(ca), i32(cg)

    def everything(a, g, na, ng):
        out = [M.chroma_distance(a, g, na, ng, pad_mode), M.chroma_similarity(g, a, ng, na, pad_mode), M.pitch_correlation(a, g, na, ng, pad_mode),
               M.pitch_mean(a, na, pad_mode)]
        for n_fft, hop in SETTINGS:
            out += [M.estimate_tuning(a, na, n_fft, hop, pad_mode), M.chroma_stft(a, na, n_fft, hop, pad_mode)]
        return out

    full = everything(a, g, na, ng)
    for b in range(F.B):
        # row b of the padded batch is the clip alone at B = 1, bit for bit
        xa, xg = a[b:b + 1, :ca[b]].contiguous(), g[b:b + 1, :cg[b]].contiguous()
        for k, (one, many) in enumerate(zip(everything(xa, xg, None, None), full)):
            T = one.shape[-1]
            assert torch.equal(one[0], many[b][..., :T] if many.dim() > 1 else many[b]), (b, k)
            if many.dim() > 1:
                assert not many[b][..., T:].any() and bool(torch.isfinite(many[b]).all()), (b, k)
    # NaN behind every clip's end changes nothing; repeats are bitwise equal
    an, gn = waves(fill=float("nan"))
    for one, many in zip(everything(an, gn, na, ng), full):
        assert torch.equal(one, many)
    for one, many in zip(everything(a, g, na, ng), full):
        assert torch.equal(one, many)
    # device counts outside the range equal the clamped ones; no counts: the rows are full
    lo = {"constant": (1, 1), "reflect": (1025, 513)}[pad_mode]                      # at n_fft 2048, at n_fft 1024
    wild = everything(a, g, i32([0, -5, F.N_MAX + 9, ca[3]]), ng)
    for lo_k, which in ((lo[0], (0, 2, 3, 4, 5)), (lo[1], (1, 6, 7))):
        clamped = everything(a, g, i32([lo_k, lo_k, F.N_MAX, ca[3]]), ng)
        for k in which:
            assert torch.equal(wild[k], clamped[k]), k
    fullc = i32([F.N_MAX] * F.B)
    for x, y in zip(everything(a, g, None, None), everything(a, g, fullc, fullc)):
        assert torch.equal(x, y)


def test_wrappers_refuse_bad_arguments_on_the_device():
    ok = torch.zeros(2, 3000, device=DEV)
    for kw in (dict(n_fft=2048, hop_length=256), dict(n_fft=512, hop_length=128), dict(pad_mode="edge")):
        with pytest.raises(ValueError):
            M.chroma_stft(ok, **kw)
    with pytest.raises(ValueError, match="1025"):
        M.chroma_distance(ok, torch.zeros(2, 1024, device=DEV), pad_mode="reflect")
    with pytest.raises(ValueError, match="tuning"):
        M.chroma_stft(ok, tuning=torch.zeros(3, device=DEV))
    assert M.chroma_stft(ok).shape == (2, 12, 6) and M.chroma_stft(ok, n_fft=1024, hop_length=256).shape == (2, 12, 12)


# ---- transfer_and_score(..., chroma=True) ----------------------------------------------------------------------------------------------
def test_transfer_and_score_with_chroma():
    """In bf16, where two runs of the session agree bit for bit (test_gpu_ragged_wave: the f32 session has run-to-run noise of
    5.3e-7, so 'bit-equal to chroma=False' can only be asked of bf16).  The session is test_gpu_mfcc's, the smallest the ragged-wave
    tests use."""
    from test_gpu_ragged_wave import _seeded, padded_batch
    from test_ragged_wave_cpu import NS
    from oracle import seeded_params as sp
    config.set_compute_dtype(torch.bfloat16)
    try:
        enc, dec = _seeded("content", ast_amd.ContentEncoder), _seeded("decoder", ast_amd.Decoder)
        cls = sp.seeded_normal((2, 256), 7710).to(DEV)
        eager, graph = StyleTransferSession(enc, dec, use_graph=False), StyleTransferSession(enc, dec, use_graph=True)
        for order in ([0, 2], [2, 0]):                                    # 85 760 and 36 708 samples, then swapped
            wav, n = padded_batch(order)
            assert n.tolist() == [NS[b] for b in order]
            for sess in (eager, graph):
                plain = sess.transfer_and_score(wav, cls, n_samples=n)
                want = tuple(t.clone() for t in plain[:3]) + ({k: v.clone() for k, v in plain[3].items()},)
                assert sorted(want[3]) == ["mse_spectrogram"]
                res = sess.transfer_and_score(wav, cls, n_samples=n, chroma=True)
                assert len(res) == 4 and sorted(res[3]) == ["chroma_similarity", "mse_spectrogram"]
                for got, exp in zip(res[:3], want[:3]):                   # the first three outputs and the old scores: bit-equal to chroma=False
                    assert torch.equal(got, exp)
                assert torch.equal(res[3]["mse_spectrogram"], want[3]["mse_spectrogram"])
                d = res[3]["chroma_similarity"]
                print(f"transfer_and_score(chroma=True), {'graph' if sess is graph else 'eager'}, order {order}: chroma_similarity {d.tolist()}")
                assert d.shape == (2,) and bool(torch.isfinite(d).all()) and bool((d.abs() <= 1).all())
                assert torch.equal(d, M.chroma_similarity(res[0], wav, res[2], n))                     # the stand-alone function, bit for bit
        assert len(graph._graphs) == 2                                    # with and without chroma: the swapped batch replayed both
    finally:
        config.set_compute_dtype(torch.float32)
