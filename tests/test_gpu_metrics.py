"""Spectrogram metrics on the device (ast_amd/metrics.py, csrc/metrics.hip): mse_spectrogram, band_energy and
instrumentation_similarity for ragged batches, and StyleTransferSession.transfer_and_score.

Reference and bounds (tests/metrics_ref.py): the float64 restatement of librosa.stft's documented defaults.  The tolerance is
10 x the float32 floor -- the same restatement evaluated in float32 on the CPU against its float64 form, on the same clips:
    constant: floor mse 2.5e-7 (relative), energy 1.7e-7 (of a row's peak), similarity 1.4e-8 (absolute); the kernels: 8.5e-8, 1.5e-7, 1.1e-8
    reflect:  floor mse 9.8e-8, energy 1.7e-7, similarity 2.2e-8;                                        the kernels: 8.9e-8, 1.5e-7, 3.4e-8
(the floor is measured where the test runs and moves a little with the host's FFT library: 5.7e-8 for the reflect MSE elsewhere)
Row 1 of the constant-mode fixture holds one sample: its energy vector is constant to rounding, so Pearson's r is 0 / 0 up to
rounding noise in the float64 restatement as well (the reference's own formula is ill-conditioned there); for such rows
(metrics_ref.conditioned_rows) the similarity is only required to be finite and inside [-1, 1], every other quantity of the row is
compared as usual."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import ast_amd
    from ast_amd import _lib, config
    from ast_amd import metrics as M
    from ast_amd import utilityFunctions as U
    from ast_amd.infer import StyleTransferSession

import metrics_ref as R

DEV = "cuda"
MODES = ["constant", "reflect"]


def i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def waves(fill=None, pad_mode="constant"):
    """the fixture on the device; fill: that value behind every clip's end (as the device clamps the counts)"""
    a, g = (t.to(DEV).clone() for t in R.fixture_waves())
    if fill is not None:
        lo = 1025 if pad_mode == "reflect" else 1
        for b in range(R.B):
            a[b, max(R.COUNTS[pad_mode][b], lo):] = fill
            g[b, max(R.N_GENERATED[b], lo):] = fill
    return a, g


def test_fixture_reaches_every_run_case():
    run = _lib.lib().ast_band_energy_run_frames()
    frames = sorted({R.n_frames(n, R.BAND_HOP) for counts in R.COUNTS.values() for n in counts})
    assert any(T < run for T in frames), "a clip with fewer frames than one run"
    assert any(T >= run and T % run == 0 for T in frames), "a clip of exactly whole runs"
    assert any(T > run and T % run for T in frames), "a clip with a ragged last run"


@pytest.mark.parametrize("pad_mode", MODES)
def test_metrics_match_the_float64_restatement(pad_mode):
    a, g = waves()
    na, ng = i32(R.COUNTS[pad_mode]), i32(R.N_GENERATED)
    ref, bound, floor = R.references(pad_mode), R.bounds(pad_mode), R.f32_floor(pad_mode)
    mse = M.mse_spectrogram(a, g, na, ng, pad_mode).cpu().double()
    ea, eg = M.band_energy(a, na, pad_mode).cpu(), M.band_energy(g, ng, pad_mode).cpu()
    sim = M.instrumentation_similarity(a, g, na, ng, pad_mode).cpu().double()
    assert mse.shape == (R.B,) and ea.shape == (R.B, 1025) and sim.shape == (R.B,) and ea.dtype == torch.float32
    e_mse = max(abs(float(mse[b] / ref["mse"][b]) - 1) for b in range(R.B))
    e_en = max(R._rel(e[b], ref[k][b]) for e, k in ((ea, "energy"), (eg, "energy_gen")) for b in range(R.B))
    ok = R.conditioned_rows(pad_mode)
    e_sim = max(abs(float(sim[b] - ref["sim"][b])) for b in ok)
    print(f"{pad_mode}: mse {e_mse:.3g} (floor {floor['mse']:.3g}, bound {bound['mse']:.3g}), energy {e_en:.3g} (floor {floor['energy']:.3g}, "
          f"bound {bound['energy']:.3g}), similarity {e_sim:.3g} on rows {ok} (floor {floor['sim']:.3g}, bound {bound['sim']:.3g})")
    assert e_mse <= bound["mse"] and e_en <= bound["energy"] and e_sim <= bound["sim"]
    assert bool(torch.isfinite(sim).all()) and float(sim.abs().max()) <= 1.0
    # the constant-mode counts also run with the reflect-mode clips' counts (a clip of exactly whole runs in this mode too)
    if pad_mode == "constant":
        a_cpu, _ = R.fixture_waves()
        got = M.band_energy(a, i32(R.COUNTS["reflect"]), "constant").cpu()
        for b in range(R.B):
            assert R._rel(got[b], R.band_energy(a_cpu[b, :R.COUNTS["reflect"][b]], "constant")) <= bound["energy"], b


@pytest.mark.parametrize("pad_mode", MODES)
def test_known_answers(pad_mode):
    a, _ = waves()
    na = i32(R.COUNTS[pad_mode])
    bound = R.bounds(pad_mode)
    assert M.mse_spectrogram(a, a, na, na, pad_mode).tolist() == [0.0] * R.B                       # exactly
    assert M.mse_spectrogram(a, a.clone(), None, na, pad_mode).tolist() == [0.0] * R.B
    ok = R.conditioned_rows(pad_mode)
    same, twice = M.instrumentation_similarity(a, a, na, na, pad_mode).cpu(), M.instrumentation_similarity(a, 2 * a, na, na, pad_mode).cpu()
    print(f"{pad_mode}: similarity(a, a) - 1 = {(same[ok] - 1).tolist()}, similarity(a, 2a) - 1 = {(twice[ok] - 1).tolist()}")
    assert float((same[ok] - 1).abs().max()) <= bound["sim"] and float((twice[ok] - 1).abs().max()) <= bound["sim"]
    zero = torch.zeros(2, 5000, device=DEV)
    assert M.instrumentation_similarity(zero, zero, pad_mode=pad_mode).tolist() == [0.0, 0.0]       # the NaN rule
    assert M.instrumentation_similarity(zero, a[:2], pad_mode=pad_mode).tolist() == [0.0, 0.0]
    assert M.mse_spectrogram(zero, zero, pad_mode=pad_mode).tolist() == [0.0, 0.0]
    # a unit sine at k * 22050 / 1024 Hz: the arg-max of the band energies is bin 2 k (bins of 22050 / 2048 Hz)
    ks = [3, 100, 411]
    t = torch.arange(22050, dtype=torch.float64)
    sines = torch.stack([torch.sin(2 * torch.pi * k / 1024 * t) for k in ks]).float().to(DEV)
    assert M.band_energy(sines, pad_mode=pad_mode).argmax(dim=1).tolist() == [2 * k for k in ks]


def test_mse_against_the_front_end():
    """mse_spectrogram(a, 0, reflect) * 513 * T is the sum of |STFT|^2, which the front end's kernel (get_STFT) delivers as well.
    Tolerance by the same rule: 10 x the float32 floor of that sum (float32 against float64 restatement), relative."""
    a_cpu, _ = R.fixture_waves()
    a, _ = waves()
    for b, n in ((0, R.N_MAX), (3, 20481)):
        clip = a[b:b + 1, :n].contiguous()
        T = 1 + n // 256
        got = float(M.mse_spectrogram(clip, torch.zeros_like(clip), pad_mode="reflect")[0].double() * 513 * T)
        st = U.get_STFT(clip[0]).double()
        assert st.shape == (2, T, 513)
        front = float((st ** 2).sum())
        want = float((R.magnitudes(a_cpu[b, :n], 1024, 256, "reflect") ** 2).sum())
        f32 = float((R.magnitudes(a_cpu[b, :n], 1024, 256, "reflect", torch.float32) ** 2).sum())
        floor = abs(f32 / want - 1)
        floor = max(floor, 2.0 ** -24)          # a float32 sum cannot be held to less than half an ulp of itself
        print(f"row {b}: metrics kernel against the front end {abs(got / front - 1):.3g}, against float64 {abs(got / want - 1):.3g}, "
              f"front end against float64 {abs(front / want - 1):.3g}; float32 floor {floor:.3g}")
        assert abs(got / front - 1) <= 10 * floor and abs(got / want - 1) <= 10 * floor


@pytest.mark.parametrize("pad_mode", MODES)
def test_ragged_contract(pad_mode):
    a, g = waves()
    counts, lo_m, lo_b = R.COUNTS[pad_mode], (513 if pad_mode == "reflect" else 1), (1025 if pad_mode == "reflect" else 1)
    na, ng = i32(counts), i32(R.N_GENERATED)
    mse, ea, sim = M.mse_spectrogram(a, g, na, ng, pad_mode), M.band_energy(a, na, pad_mode), M.instrumentation_similarity(a, g, na, ng, pad_mode)
    # row b of the padded batch is the clip alone at B = 1, bit for bit
    for b in range(R.B):
        ca, cg = a[b:b + 1, :max(counts[b], lo_m)].contiguous(), g[b:b + 1, :max(R.N_GENERATED[b], lo_m)].contiguous()
        assert torch.equal(M.mse_spectrogram(ca, cg, pad_mode=pad_mode), mse[b:b + 1]), b
        ca, cg = a[b:b + 1, :max(counts[b], lo_b)].contiguous(), g[b:b + 1, :max(R.N_GENERATED[b], lo_b)].contiguous()
        assert torch.equal(M.band_energy(ca, pad_mode=pad_mode), ea[b:b + 1]), b
        assert torch.equal(M.instrumentation_similarity(ca, cg, pad_mode=pad_mode), sim[b:b + 1]), b
    # NaN behind every clip's end changes nothing
    an, gn = waves(fill=float("nan"), pad_mode=pad_mode)
    if pad_mode == "reflect":                   # the MSE clamps to 513, below the 1025 that `waves` keeps: fill from there for it
        am, gm = a.clone(), g.clone()
        for b in range(R.B):
            am[b, max(counts[b], 513):] = float("nan")
            gm[b, max(R.N_GENERATED[b], 513):] = float("nan")
    else:
        am, gm = an, gn
    assert torch.equal(M.mse_spectrogram(am, gm, na, ng, pad_mode), mse)
    assert torch.equal(M.band_energy(an, na, pad_mode), ea) and torch.equal(M.instrumentation_similarity(an, gn, na, ng, pad_mode), sim)
    # device counts outside the range equal the clamped ones
    wild, clamped = i32([0, -5, R.N_MAX + 9, counts[3]]), i32([lo_b, lo_b, R.N_MAX, counts[3]])
    assert torch.equal(M.band_energy(a, wild, pad_mode), M.band_energy(a, clamped, pad_mode))
    assert torch.equal(M.instrumentation_similarity(a, g, wild, ng, pad_mode), M.instrumentation_similarity(a, g, clamped, ng, pad_mode))
    clamped = i32([lo_m, lo_m, R.N_MAX, counts[3]])
    assert torch.equal(M.mse_spectrogram(a, g, wild, ng, pad_mode), M.mse_spectrogram(a, g, clamped, ng, pad_mode))
    assert torch.equal(M.mse_spectrogram(a, g, ng, wild, pad_mode), M.mse_spectrogram(a, g, ng, clamped, pad_mode))
    # repeats are bitwise equal
    for _ in range(2):
        assert torch.equal(M.mse_spectrogram(a, g, na, ng, pad_mode), mse) and torch.equal(M.band_energy(a, na, pad_mode), ea)
        assert torch.equal(M.instrumentation_similarity(a, g, na, ng, pad_mode), sim)
    # no counts: the rows are full
    full = i32([R.N_MAX] * R.B)
    assert torch.equal(M.mse_spectrogram(a, g, pad_mode=pad_mode), M.mse_spectrogram(a, g, full, full, pad_mode))
    assert torch.equal(M.mse_spectrogram(a, g, na, None, pad_mode), M.mse_spectrogram(a, g, na, full, pad_mode))
    assert torch.equal(M.band_energy(a, None, pad_mode), M.band_energy(a, full, pad_mode))
    assert torch.equal(M.instrumentation_similarity(a, g, None, None, pad_mode), M.instrumentation_similarity(a, g, full, full, pad_mode))
    # rows of different widths
    assert torch.equal(M.mse_spectrogram(a, g[:, :30000].contiguous(), na, i32([30000, 30000, 777, 20480]), pad_mode),
                       M.mse_spectrogram(a, g, na, i32([30000, 30000, 777, 20480]), pad_mode))


# ---- transfer_and_score ------------------------------------------------------------------------------------------------------------
def _score_check(bound):
    from test_gpu_ragged_wave import _seeded, padded_batch, rel_err
    from test_ragged_wave_cpu import NS
    from oracle import seeded_params as sp
    enc, dec = _seeded("content", ast_amd.ContentEncoder), _seeded("decoder", ast_amd.Decoder)
    cls = sp.seeded_normal((2, 256), 7710).to(DEV)
    plain = StyleTransferSession(enc, dec, use_graph=False)
    eager, graph = StyleTransferSession(enc, dec, use_graph=False), StyleTransferSession(enc, dec, use_graph=True)
    for order in ([0, 2], [2, 0]):                                    # 85 760 and 36 708 samples, then swapped
        wav, n = padded_batch(order)
        ref_w, ref_n = padded_batch(order[::-1])
        assert n.tolist() == [NS[b] for b in order] and sorted(n.tolist()) == [36708, 85760]
        want = tuple(t.clone() for t in plain.transfer(wav, cls, n_samples=n))
        for sess in (eager, graph):
            res = sess.transfer_and_score(wav, cls, n_samples=n, reference=ref_w, n_reference=ref_n)
            assert len(res) == 4 and sorted(res[3]) == ["instrumentation_similarity", "mse_spectrogram"]
            wave, out, lengths = (t.clone() for t in res[:3])
            scores = {k: v.clone() for k, v in res[3].items()}
            assert wave.shape == want[0].shape and out.shape == want[1].shape and torch.equal(lengths, want[2])
            ew, eo = rel_err(wave, want[0]), rel_err(out, want[1])
            print(f"transfer_and_score ({config.compute_dtype}, {'graph' if sess is graph else 'eager'}, order {order}): against transfer "
                  f"waveforms {ew:.3g}, sections {eo:.3g} (bound {bound:.3g}); scores {({k: v.tolist() for k, v in scores.items()})}")
            if bound == 0.0:
                assert torch.equal(wave, want[0]) and torch.equal(out, want[1])
            else:
                assert ew <= bound and eo <= bound
            # the scores are the stand-alone functions on these outputs, bit for bit
            assert torch.equal(scores["mse_spectrogram"], M.mse_spectrogram(wav, wave, n, lengths))
            assert torch.equal(scores["instrumentation_similarity"], M.instrumentation_similarity(wave, ref_w, lengths, ref_n))
            assert scores["mse_spectrogram"].shape == (2,) and bool(torch.isfinite(scores["mse_spectrogram"]).all())
            assert bool((scores["mse_spectrogram"] > 0).all()) and float(scores["instrumentation_similarity"].abs().max()) <= 1.0
            only = sess.transfer_and_score(wav, cls, n_samples=n)     # without a reference: the MSE alone
            assert sorted(only[3]) == ["mse_spectrogram"]
            assert torch.equal(only[3]["mse_spectrogram"], M.mse_spectrogram(wav, only[0], n, only[2]))
        assert len(graph._graphs) == 2                                # one with a reference, one without: every mix of lengths replays them


def test_transfer_and_score_f32():
    from test_gpu_ragged_wave import BOUND_SESSION_F32
    config.set_compute_dtype(torch.float32)
    _score_check(BOUND_SESSION_F32)


def test_transfer_and_score_bf16():
    config.set_compute_dtype(torch.bfloat16)
    try:
        _score_check(0.0)
    finally:
        config.set_compute_dtype(torch.float32)
