"""Dataset screening on the device (ast_amd.frame_rms, silence_ratio, clip_rms, sound_ratio, mfcc_mean, rms_normalize, screen;
csrc/curation.hip).

Reference (tests/curation_ref.py): the float64 restatement of librosa's and pydub's definitions -- explicit padding and framing, the
mean of the per-frame DCT.  Continuous outputs (frame RMS, clip level, MFCC means, normalised waves; each error relative to the
clip's peak value) must lie within 10 x the float32 floor, the error of the float32 twin that follows the kernels' summation orders,
computed where the test runs.  Integer outputs (silent frames, sound-window masks, frame counts) must equal the restatement exactly;
tests/test_curation_cpu.py shows that no fixture frame or window lies near its threshold, so nothing is excluded.  Every input has
NaN behind each clip's end.  The figures reached on the MI355X are in DESIGN 7, "Dataset screening"."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import ast_amd
    from ast_amd import curation as Cu
    from ast_amd import metrics as M

import curation_ref as F

DEV = "cuda"


def i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def waves(pad_mode, fill=float("nan")):
    """the fixture on the device, `fill` behind every clip's end"""
    w = F.fixture_waves().to(DEV).clone()
    for b in range(F.B):
        w[b, F.COUNTS[pad_mode][b]:] = fill
    return w


@pytest.mark.parametrize("pad_mode", F.MODES)
def test_values_match_the_float64_restatement(pad_mode):
    counts, ref, bound, floor = F.COUNTS[pad_mode], F.references(pad_mode), F.bounds(pad_mode), F.f32_floor(pad_mode)
    w, ns = waves(pad_mode), i32(counts)
    rms = Cu.frame_rms(w, ns, pad_mode).cpu()
    T_max = F.n_frames(F.N_MAX)
    assert rms.shape == (F.B, T_max) and rms.dtype == torch.float32
    got = dict(rms=[rms[b, :F.n_frames(counts[b])].numpy() for b in range(F.B)], mfcc={})
    for b in range(F.B):
        assert float(rms[b, F.n_frames(counts[b]):].abs().sum()) == 0.0 and bool(torch.isfinite(rms[b]).all()), b    # exactly 0 behind the clip
    for sr in F.RATES:
        c = Cu.mfcc_mean(w, ns, sample_rate=sr, pad_mode=pad_mode).cpu()
        assert c.shape == (F.B, F.N_MFCC) and c.dtype == torch.float32
        got["mfcc"][sr] = list(c.numpy())
    # the level and the gain take the clip as it is: "constant" counts whatever the frames' pad mode
    e = F.errors(dict(got, level=ref["level"], norm=ref["norm"]), pad_mode)
    print(f"{pad_mode}: frame RMS {e['rms']:.3g} (floor {floor['rms']:.3g}, bound {bound['rms']:.3g}), MFCC mean {e['mfcc']:.3g} "
          f"(floor {floor['mfcc']:.3g}, bound {bound['mfcc']:.3g})")
    assert e["rms"] <= bound["rms"] and e["mfcc"] <= bound["mfcc"], e
    # silent frames, frame counts: exactly
    res = Cu.screen(w, ns, pad_mode=pad_mode)
    assert res["n_frames"].tolist() == [F.n_frames(n) for n in counts]
    silent = [int((rms[b, :F.n_frames(counts[b])] < F.SILENCE_RMS).sum()) for b in range(F.B)]
    assert silent == ref["silent"]
    ratio = Cu.silence_ratio(w, ns, pad_mode=pad_mode).cpu()
    want = torch.tensor([s / F.n_frames(n) for s, n in zip(ref["silent"], counts)], dtype=torch.float64).float()
    assert torch.equal(ratio, want)
    # ... and equal to the count over the device's own frame_rms
    own = torch.tensor([float((rms[b, :F.n_frames(counts[b])] < F.SILENCE_RMS).sum()) / F.n_frames(counts[b]) for b in range(F.B)],
                       dtype=torch.float64).float()
    assert torch.equal(ratio, own)
    assert float(ratio[F.ZERO_ROW]) == 1.0 and 0 < float(ratio[F.MIX_ROW]) < 1 and float(ratio[9]) == 0.0
    # another threshold counts other frames
    assert torch.equal(Cu.silence_ratio(w, ns, threshold=0.1, pad_mode=pad_mode).cpu(),
                       torch.tensor([float((rms[b, :F.n_frames(counts[b])] < np.float32(0.1)).sum()) / F.n_frames(counts[b]) for b in range(F.B)],
                                    dtype=torch.float64).float())


def test_level_gain_and_windows_match_the_float64_restatement():
    pad_mode = "constant"
    counts, ref, bound, floor = F.COUNTS[pad_mode], F.references(pad_mode), F.bounds(pad_mode), F.f32_floor(pad_mode)
    w, ns = waves(pad_mode), i32(counts)
    level = Cu.clip_rms(w, ns).cpu()
    out = Cu.rms_normalize(w, ns)
    assert out.shape == w.shape and out.dtype == torch.float32 and out.data_ptr() != w.data_ptr()
    outc = out.cpu()
    got = dict(rms=ref["rms"], mfcc=ref["mfcc"], level=[float(v) for v in level], norm=[outc[b, :counts[b]].numpy() for b in range(F.B)])
    e = F.errors(got, pad_mode)
    print(f"clip level {e['level']:.3g} (floor {floor['level']:.3g}, bound {bound['level']:.3g}), normalised waves {e['norm']:.3g} "
          f"(floor {floor['norm']:.3g}, bound {bound['norm']:.3g})")
    assert e["level"] <= bound["level"] and e["norm"] <= bound["norm"], e
    for b in range(F.B):
        assert float(outc[b, counts[b]:].abs().sum()) == 0.0 and bool(torch.isfinite(outc[b]).all()), b               # exactly 0 behind the clip
    # the all-zero clip: level 0, returned unchanged; a one-sample clip's level is the sample
    assert float(level[F.ZERO_ROW]) == 0.0 and not outc[F.ZERO_ROW].any()
    assert float(level[0]) == pytest.approx(abs(float(F.fixture_waves()[0, 0])), rel=1.2e-7)
    assert torch.allclose(Cu.clip_rms(out, ns).cpu()[[b for b in range(F.B) if b != F.ZERO_ROW]], torch.tensor(0.07), rtol=1e-6, atol=0)
    # in place, and another target
    w2 = w.clone()
    assert Cu.rms_normalize(w2, ns, out=w2) is w2 and torch.equal(w2, out)
    assert torch.allclose(Cu.rms_normalize(w, ns, target_rms=0.5).cpu()[9], outc[9] * (0.5 / 0.07), rtol=1e-6, atol=0)
    # sound windows: exactly
    for sr in F.RATES:
        win = sr // 10
        mask, ratio = Cu.sound_windows(w, ns, sample_rate=sr).cpu(), Cu.sound_ratio(w, ns, sample_rate=sr).cpu()
        assert mask.shape == (F.B, F.N_MAX // win) and mask.dtype == torch.int32 and ratio.dtype == torch.float32
        for b in range(F.B):
            W = counts[b] // win
            assert mask[b, :W].tolist() == ref["sound"][sr][b].tolist(), (sr, b)
            assert int(mask[b, W:].abs().sum()) == 0
        want = [F.sound_ratio(x, sr) for x in F.clips(pad_mode)]
        assert torch.equal(ratio, torch.tensor(want, dtype=torch.float64).float())
        assert float(ratio[0]) == 0.0 and float(ratio[F.ZERO_ROW]) == 0.0 and float(ratio[9]) == 1.0 and 0 < float(ratio[F.MIX_ROW]) < 1
    # a row shorter than a window: no mask columns, ratio exactly 0
    short = w[:, :2000].contiguous()
    assert Cu.sound_windows(short).shape == (F.B, 0) and Cu.sound_ratio(short).tolist() == [0.0] * F.B
    # another threshold and another window length
    assert float(Cu.sound_ratio(w, ns, threshold_db=-70.0)[F.MIX_ROW]) == 1.0 and float(Cu.sound_ratio(w, ns, threshold_db=-30.0)[F.MIX_ROW]) == 0.0
    assert Cu.sound_windows(w, ns, frame_ms=50).shape == (F.B, F.N_MAX // 1102)


@pytest.mark.parametrize("pad_mode", F.MODES)
def test_silence_and_the_parent_route(pad_mode):
    counts, bound = F.COUNTS[pad_mode], F.bounds(pad_mode)
    w, ns = waves(pad_mode), i32(counts)
    c = Cu.mfcc_mean(w, ns, pad_mode=pad_mode).cpu().double()
    # the all-zero clip: coefficient 0 is -100 sqrt(128), the others are rounding noise around 0 (silence is decided by noise)
    peak = 100 * 128 ** 0.5
    z = c[F.ZERO_ROW]
    print(f"{pad_mode}: silent clip's coefficients {z[0]:.6f} (want {-peak:.6f}), others at most {float(z[1:].abs().max()):.3g}")
    assert abs(float(z[0]) + peak) <= bound["mfcc"] * peak and float(z[1:].abs().max()) <= bound["mfcc"] * peak
    # the parent's route: ast_amd.mfcc and a masked time-mean
    for hop in (512, 256):
        full = M.mfcc(w, ns, n_mfcc=13, hop_length=hop, pad_mode=pad_mode).cpu().double()
        mean = Cu.mfcc_mean(w, ns, hop_length=hop, pad_mode=pad_mode).cpu().double()
        worst = 0.0
        for b in range(F.B):
            T = 1 + counts[b] // hop
            other = full[b, :, :T].mean(dim=1)
            worst = max(worst, float((mean[b] - other).abs().max() / other.abs().max()))
        print(f"{pad_mode}, hop {hop}: mfcc_mean against the masked mean of ast_amd.mfcc {worst:.3g} (bound {bound['mfcc']:.3g})")
        assert worst <= bound["mfcc"]
    assert torch.equal(Cu.mfcc_mean(w, ns, n_mfcc=20, pad_mode=pad_mode)[:, :13].cpu().double(), c) and Cu.mfcc_mean(w, ns, n_mfcc=1).shape == (F.B, 1)


@pytest.mark.parametrize("pad_mode", F.MODES)
def test_screen_and_the_ragged_contract(pad_mode):
    counts, lo = F.COUNTS[pad_mode], (1025 if pad_mode == "reflect" else 1)
    w, ns = waves(pad_mode), i32(counts)

    def singles(x, n, sr=22050):
        return dict(rms_level=Cu.clip_rms(x, n), silence_ratio=Cu.silence_ratio(x, n, pad_mode=pad_mode), sound_ratio=Cu.sound_ratio(x, n, sample_rate=sr),
                    mfcc_mean=Cu.mfcc_mean(x, n, sample_rate=sr, pad_mode=pad_mode),
                    n_frames=torch.tensor([1 + max(lo, min(int(v), x.shape[1])) // 512 for v in (n.tolist() if n is not None else [x.shape[1]] * x.shape[0])],
                                          dtype=torch.int32, device=DEV))

    def everything(x, n):
        return dict(singles(x, n), rms=Cu.frame_rms(x, n, pad_mode), mask=Cu.sound_windows(x, n), norm=Cu.rms_normalize(x, n))

    def same(p, q):
        assert sorted(p) == sorted(q)
        return all(torch.equal(p[k], q[k]) for k in p)

    # screen: bit-identical to the single calls, at both rates
    for sr in F.RATES:
        res = Cu.screen(w, ns, sample_rate=sr, pad_mode=pad_mode)
        assert sorted(res) == ["mfcc_mean", "n_frames", "rms_level", "silence_ratio", "sound_ratio"] and same(res, singles(w, ns, sr))
    one = everything(w, ns)
    # NaN behind every clip's end changes nothing: zeros there give the same bits
    assert same(everything(waves(pad_mode, fill=0.0), ns), one)
    # the clips permuted within the batch give the permuted results bit for bit
    perm = [7, 3, 11, 0, 9, 5, 10, 2, 8, 1, 6, 4]
    wp, nsp = w[perm].contiguous(), i32([counts[p] for p in perm])
    assert same(everything(wp, nsp), {k: v[perm] for k, v in one.items()})
    # rows one sample wider: all but every fourth row leave the 16-byte alignment and take the other load path, with the same bits
    assert F.N_MAX % 4 == 0
    odd = torch.full((F.B, F.N_MAX + 1), float("nan"), device=DEV)
    odd[:, :F.N_MAX] = w
    got = everything(odd, ns)
    assert same({k: v for k, v in got.items() if k not in ("rms", "mask", "norm")}, {k: v for k, v in one.items() if k not in ("rms", "mask", "norm")})
    assert torch.equal(got["rms"], one["rms"]) and torch.equal(got["mask"], one["mask"]) and torch.equal(got["norm"][:, :F.N_MAX], one["norm"])
    # a clip alone at B = 1 is its row of the batch
    for b in (0, 5, 7, 9, F.MIX_ROW):
        alone = everything(w[b:b + 1, :counts[b]].contiguous(), None)
        T, W = F.n_frames(counts[b]), counts[b] // 2205
        for k in ("rms_level", "silence_ratio", "sound_ratio", "mfcc_mean", "n_frames"):
            assert torch.equal(alone[k][0], one[k][b]), (b, k)
        assert torch.equal(alone["rms"][0], one["rms"][b, :T]) and torch.equal(alone["mask"][0], one["mask"][b, :W])
        assert torch.equal(alone["norm"][0], one["norm"][b, :counts[b]])
    # device counts outside the range equal the clamped ones; no counts: the rows are full
    wz = waves(pad_mode, fill=0.25)
    # (to [1025, n] where the frames are reflect-padded, to [1, n] for the level, the gain and the windows)
    wild = everything(wz, i32([0, -5, F.N_MAX + 9] + counts[3:]))
    framed, plain = everything(wz, i32([lo, lo, F.N_MAX] + counts[3:])), everything(wz, i32([1, 1, F.N_MAX] + counts[3:]))
    for k in wild:
        assert torch.equal(wild[k], (framed if k in ("rms", "silence_ratio", "mfcc_mean", "n_frames") else plain)[k]), k
    assert same(everything(wz, None), everything(wz, i32([F.N_MAX] * F.B)))
    # repeats are bitwise equal
    assert same(everything(w, ns), one)
    # stereo rows are averaged first
    st = torch.stack([w, 3 * w], dim=1)
    assert same(Cu.screen(st, ns, pad_mode=pad_mode), Cu.screen(((w + 3 * w) * 0.5).contiguous(), ns, pad_mode=pad_mode))
    assert same(Cu.screen(w[:, None], ns, pad_mode=pad_mode), Cu.screen(w, ns, pad_mode=pad_mode))


def test_screen_in_a_graph_replays_other_lengths():
    pad_mode = "constant"
    counts = F.COUNTS[pad_mode]
    second = [counts[(b + 5) % F.B] for b in range(F.B)]
    w = waves(pad_mode, fill=0.5)                                                       # the second set reads behind the first set's ends
    ns = i32(counts)
    eager = [Cu.screen(w, i32(c), sample_rate=44100) for c in (counts, second)]         # also builds the mel table outside the capture
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        Cu.screen(w, ns, sample_rate=44100)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = Cu.screen(w, ns, sample_rate=44100)
    for c, want in zip((counts, second), eager):
        ns.copy_(i32(c))
        graph.replay()
        torch.cuda.synchronize()
        for k in want:
            assert torch.equal(res[k], want[k]), k
    assert not torch.equal(eager[0]["rms_level"], eager[1]["rms_level"])


def test_dataset_report_from_a_screened_batch():
    counts = F.COUNTS["constant"]
    w, ns = waves("constant"), i32(counts)
    names = [f"clip_{b:02d}.wav" for b in range(F.B)]
    rep = ast_amd.DatasetReport()
    rep.add(names, ast_amd.screen(w, ns), ns, 22050)
    ref = F.references("constant")
    flagged = rep.flagged()
    want = [names[b] for b in range(F.B) if ref["silent"][b] / F.n_frames(counts[b]) >= 0.3]
    assert [f for f, _ in flagged] == want and names[F.ZERO_ROW] in want
    # the lines of summarize_statistics, its format strings on the device's own values (their accuracy is the tests' above)
    res = ast_amd.screen(w, ns)
    text = rep.summary("Dataset 1")
    assert f"• Files analyzed: {F.B}" in text and f"• Average RMS: {np.mean(res['rms_level'].double().cpu().numpy()):.4f}" in text
    assert f"• Average duration: {np.mean([c / 22050 for c in counts]):.2f} sec" in text and "• Unique sample rates: {22050}" in text
    assert f"(first coefficient).: {np.mean(res['mfcc_mean'][:, 0].double().cpu().numpy()):.2f}" in text
    assert abs(np.mean(res["rms_level"].double().cpu().numpy()) - np.mean(ref["level"])) < 1e-6
