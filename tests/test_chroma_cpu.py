"""Chroma and pitch metrics without a GPU: what the float64 restatement (tests/chroma_ref.py) that tests/test_gpu_chroma.py checks
the kernels against is pinned to -- properties of the filter bank, known answers for sines and silence, Pearson's r to
scipy.stats.pearsonr --, the conditions of the fixture that the GPU test relies on, and that the C entries and the Python wrappers
refuse bad calls before any launch.  Parity with librosa's own output stays unpinned: librosa is not available."""
import ctypes

import numpy as np
import pytest
import scipy.stats
import torch

import ast_amd
from ast_amd import _lib
from ast_amd import metrics as M

import chroma_ref as F

FAKE = 0x10000                                            # an aligned non-null pointer; nothing dereferences it
MODES = ["constant", "reflect"]


def sine(f, n=12000):
    return np.sin(2 * np.pi * f * np.arange(n) / F.SR).astype(np.float32)


def test_band_is_derived_from_the_two_inequalities():
    assert F.band(2048) == (14, 371) and F.band(1024) == (7, 185)
    lo, hi = ctypes.c_int32(), ctypes.c_int32()
    for n_fft in (2048, 1024):
        assert _lib.lib().ast_pitch_band(n_fft, ctypes.byref(lo), ctypes.byref(hi)) == 0 and (lo.value, hi.value) == F.band(n_fft)
    assert _lib.lib().ast_pitch_band(512, ctypes.byref(lo), ctypes.byref(hi)) != 0


def test_filter_bank_columns_have_unit_norm_without_the_octave_weighting():
    for n_fft in (2048, 1024):
        for tuning in (0.0, 0.13, -0.5):
            w = F.chroma_filters(n_fft, tuning, octave=False)
            assert w.shape == (12, 1 + n_fft // 2) and np.abs(np.sqrt((w * w).sum(axis=0)) - 1).max() < 1e-12
            full = F.chroma_filters(n_fft, tuning)
            assert np.all(full >= 0) and np.all(full.max(axis=0) <= 1)


def test_sines_land_in_their_rows():
    for n_fft, hop in (F.WIDE, F.NARROW):
        a, c = F.chroma_stft(sine(440.0), n_fft, hop), F.chroma_stft(sine(261.63), n_fft, hop)
        assert np.all(a[:, 2:-2].argmax(axis=0) == 9) and np.all(c[:, 2:-2].argmax(axis=0) == 0)       # A, C
        assert a.max() == 1.0 and a.min() >= 0
    p = F.pitch_mean(sine(440.0))
    assert np.abs(p[2:-2] * 1025 - 440.0).max() < 0.5                                                   # one peak per frame, at 440 Hz


def test_silence():
    z = np.zeros(5000, dtype=np.float32)
    for n_fft, hop in (F.WIDE, F.NARROW):
        assert F.estimate_tuning(z, n_fft, hop) == 0.0
        c = F.chroma_stft(z, n_fft, hop)
        assert c.shape == (12, 1 + 5000 // hop) and not c.any()
    assert F.chroma_similarity(z, z) == 0.0 and F.pitch_correlation(z, z) == 0.0 and F.chroma_distance(z, z) == 0.0
    assert F.chroma_similarity(z, F.tones(F.TONES[0], 5)) == 0.0


def test_raising_every_tone_raises_the_tuning():
    """Every tone of the fixture raised by 0.10 semitone raises the estimated tuning, taken around the circle of one semitone, by
    0.10 to within 0.06.  Measured here over the fixture's 8 clips, both settings and both pad modes (32 estimates): 10 move by
    0.11 and 22 by 0.05, none by anything else.  The 0.11 is the 0.01 bin.  The 0.05 is the bias of piptrack's parabola, which is
    fitted to the POWER spectrum of a Hann window and, for a tone a little off a bin centre, returns about half the true offset:
    the fixture's tones sit on bin centres, the raised ones 0.05 to 0.7 of a bin above, and where the low partials (a tenth of
    a semitone is 0.05 of a bin there) fill the fullest bin, the estimate moves by half the raise.  Asserted: the largest
    measured deviation, 0.05, plus one bin."""
    moved = []
    for pm in MODES:
        for n_fft, hop in (F.WIDE, F.NARROW):
            for b in range(F.B):
                for j, count in ((0, F.COUNTS[b]), (1, F.N_GENERATED[b])):
                    x0, x1 = F.fixture_waves()[j][b, :count], F.fixture_waves(0.10)[j][b, :count]
                    d = F.estimate_tuning(x1, n_fft, hop, pm) - F.estimate_tuning(x0, n_fft, hop, pm)
                    moved.append((d + 0.5) % 1.0 - 0.5)                 # 0.45 + 0.10 comes back as -0.45
    moved = np.round(np.array(moved), 6)
    print("moved by", {float(v): int((moved == v).sum()) for v in np.unique(moved)})
    assert np.abs(moved - 0.10).max() <= 0.06 + 1e-9


def test_pearson_agrees_with_scipy():
    rng = np.random.default_rng(3)
    x, y = rng.standard_normal(200), rng.standard_normal(200)
    y += 0.5 * x
    d = x - x.mean(), y - y.mean()
    assert abs(F.pearson(x, y) - (d[0] * d[1]).sum() / np.sqrt((d[0] ** 2).sum() * (d[1] ** 2).sum())) < 1e-14
    assert F.pearson(x, y) == float(scipy.stats.pearsonr(x, y)[0])
    assert np.isnan(F.pearson(np.ones(5), x[:5])) and np.isnan(F.pearson(x[:1], y[:1]))


@pytest.mark.parametrize("pad_mode", MODES)
def test_fixture_conditions_the_gpu_test_relies_on(pad_mode):
    """from the reference alone: the float32 twin estimates the float64 tuning on every row, and the fullest bin of every
    histogram leads the runner-up by more than twice the allowance A = max(4, 10 x the twin's L1 histogram difference); one clip
    has an even and one an odd count of peaks"""
    ref, f32 = F.references(pad_mode), F.twin(pad_mode)
    parity = set()
    for s in (F.WIDE, F.NARROW):
        for b in range(F.B):
            for j in range(2):
                i, k = ref["info", s][b][j], f32["info", s][b][j]
                top = np.sort(i["hist"])[::-1]
                A = F.allowance(pad_mode, s, b, j)
                print(pad_mode, s, b, j, "tuning", round(i["tuning"], 2), "peaks", i["n"], "kept", i["kept"], "lead", top[0] - top[1], "A", A)
                assert k["tuning"] == i["tuning"], (s, b, j)
                assert top[0] - top[1] > 2 * A, (s, b, j, top[:3], A)
                assert abs(k["n"] - i["n"]) <= A
                parity.add(i["n"] % 2)
    assert parity == {0, 1}
    fl = F.f32_floor(pad_mode)
    print(pad_mode, "floors", fl)
    assert all(0 < v < 1e-4 for v in fl.values())


def test_fixture_reaches_every_run_case():
    run = _lib.lib().ast_chroma_run_frames()
    for hop in (512, 256):
        frames = sorted({1 + n // hop for n in F.COUNTS + F.N_GENERATED})
        assert any(T < run for T in frames) and any(T > run and T % run for T in frames) and any(T % run == 0 for T in frames), (hop, frames)
    assert min(F.COUNTS + F.N_GENERATED) >= 1025                                     # every clip reflect-pads at n_fft 2048


def test_entries_are_declared_and_exported():
    for name in ("ast_chroma_run_frames", "ast_pitch_band", "ast_tuning_debug_words", "ast_tuning_ws_floats", "ast_tuning_len", "ast_chroma_len",
                 "ast_chroma_distance_ws_floats", "ast_chroma_distance_len", "ast_chroma_similarity_ws_floats", "ast_chroma_similarity_len",
                 "ast_pitch_mean_len", "ast_pitch_correlation_ws_floats", "ast_pitch_correlation_len"):
        assert name in _lib.EXPORTS and name in _lib._SIGS and hasattr(_lib.lib(), name)
    for name in ("estimate_tuning", "chroma_stft", "chroma_distance", "chroma_similarity", "pitch_mean", "pitch_correlation"):
        assert getattr(ast_amd, name) is getattr(M, name)


def test_workspace_counts():
    lib = _lib.lib()
    assert lib.ast_tuning_debug_words() == 103

    def peaks(B, n, n_fft):
        lo, hi = F.band(n_fft)
        return 2 * B * (1 + n // (n_fft // 4)) * (hi - lo + 1)

    for n_fft in (2048, 1024):
        assert lib.ast_tuning_ws_floats(4, 12000, n_fft) == peaks(4, 12000, n_fft)
    assert lib.ast_tuning_ws_floats(4, 12000, 512) == 0 and lib.ast_tuning_ws_floats(0, 5, 2048) == 0
    assert lib.ast_chroma_distance_ws_floats(4, 12000, 9000) == peaks(4, 12000, 2048) + 8 + 4 * 12 * (24 + 18)
    assert lib.ast_chroma_similarity_ws_floats(4, 9000, 12000) == peaks(4, 12000, 1024) + 8 + 4 * 12 * (36 + 47)
    assert lib.ast_pitch_correlation_ws_floats(4, 12000, 9000) == 4 * (24 + 18)
    assert lib.ast_pitch_correlation_ws_floats(4, 0, 9000) == 0 and lib.ast_chroma_distance_ws_floats(0, 5, 5) == 0
    big = 2 ** 31 - 1
    assert lib.ast_tuning_ws_floats(65535, big, 1024) == peaks(65535, big, 1024)     # no 32-bit arithmetic on the way


def _refused(rc, entry, needle):
    err = _lib.lib().ast_last_error()
    assert rc != 0 and entry in err and needle in err, (rc, err)


def test_entries_refuse_bad_arguments():
    lib = _lib.lib()
    need = lib.ast_tuning_ws_floats(4, 12000, 2048)

    def tuning(**kw):
        a = dict(w=FAKE, B=4, n=12000, cut=12000, n_fft=2048, hop=512, pad=0, ws=FAKE, wsn=need, out=FAKE)
        a.update(kw)
        return lib.ast_tuning_len(a["w"], a["B"], a["n"], None, None, a["cut"], a["n_fft"], a["hop"], a["pad"], a["ws"], a["wsn"], a["out"], None, None)

    for kw, needle in ((dict(w=None), b"null"), (dict(out=None), b"null"), (dict(B=0), b"bad shape"), (dict(B=65536), b"bad shape"),
                       (dict(n=0), b"bad shape"), (dict(cut=0), b"bad shape"), (dict(hop=256), b"(2048, 512) or (1024, 256)"),
                       (dict(n_fft=4096), b"(2048, 512) or (1024, 256)"), (dict(pad=2), b"pad_mode"), (dict(pad=1, n=1024), b"reflect"),
                       (dict(pad=1, cut=1024), b"reflect"), (dict(n=2 ** 31 - 4096), b"too long"), (dict(ws=None), b"workspace"),
                       (dict(wsn=need - 1), b"workspace")):
        _refused(tuning(**kw), b"ast_tuning_len", needle)
    _refused(lib.ast_chroma_len(FAKE, 4, 12000, None, None, 12000, 2048, 512, 0, None, FAKE, None), b"ast_chroma_len", b"null")
    _refused(lib.ast_chroma_len(FAKE, 4, 12000, None, None, 12000, 1024, 512, 0, FAKE, FAKE, None), b"ast_chroma_len", b"(1024, 256)")
    _refused(lib.ast_pitch_mean_len(FAKE, 4, 1024, None, None, 1024, 1, FAKE, None), b"ast_pitch_mean_len", b"reflect")
    _refused(lib.ast_pitch_mean_len(FAKE, 4, 12000, None, None, 12000, 0, None, None), b"ast_pitch_mean_len", b"null")
    for entry, count, lo in ((lib.ast_chroma_distance_len, lib.ast_chroma_distance_ws_floats, 1025),
                             (lib.ast_chroma_similarity_len, lib.ast_chroma_similarity_ws_floats, 513),
                             (lib.ast_pitch_correlation_len, lib.ast_pitch_correlation_ws_floats, 1025)):
        need = count(4, 12000, 9000)
        name = entry.__name__.encode()

        def pair(**kw):
            a = dict(x=FAKE, nx=12000, y=FAKE, ny=9000, B=4, pad=0, ws=FAKE, wsn=need, out=FAKE)
            a.update(kw)
            return entry(a["x"], a["nx"], a["y"], a["ny"], a["B"], None, None, a["pad"], a["ws"], a["wsn"], a["out"], None)

        for kw, needle in ((dict(x=None), b"null"), (dict(y=None), b"null"), (dict(out=None), b"null"), (dict(B=0), b"bad shape"),
                           (dict(nx=0), b"bad shape"), (dict(ny=-3), b"bad shape"), (dict(pad=3), b"pad_mode"), (dict(pad=1, ny=lo - 1), b"reflect"),
                           (dict(pad=1, nx=lo - 1), b"reflect"), (dict(ws=None), b"workspace"), (dict(wsn=need - 1), b"workspace")):
            _refused(pair(**kw), name, needle)


def test_python_wrappers_refuse_bad_inputs():
    ok = torch.zeros(2, 3000)
    for fn, args in ((M.chroma_stft, (ok.double(),)), (M.estimate_tuning, (torch.zeros(2, 2, 3000),)), (M.pitch_mean, (torch.zeros(2, 0),)),
                     (M.chroma_distance, (ok, ok[0])), (M.chroma_similarity, (ok, torch.zeros(3, 3000))), (M.pitch_correlation, (ok.long(), ok))):
        with pytest.raises(ValueError):
            fn(*args)
    for kw in (dict(n_fft=2048, hop_length=256), dict(n_fft=1024, hop_length=512), dict(n_fft=512, hop_length=128), dict(hop_length=1024)):
        for fn in (M.chroma_stft, M.estimate_tuning):
            with pytest.raises(ValueError, match=r"\(2048, 512\) or \(1024, 256\)"):
                fn(ok, **kw)
    for fn in (M.chroma_stft, M.estimate_tuning, M.pitch_mean):
        with pytest.raises(ValueError, match="pad_mode"):
            fn(ok, pad_mode="edge")
        with pytest.raises(ValueError, match="n_samples"):
            fn(ok, torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="1025"):
        M.chroma_distance(ok, torch.zeros(2, 1024), pad_mode="reflect")
    with pytest.raises(ValueError, match="513"):
        M.chroma_similarity(ok, torch.zeros(2, 512), pad_mode="reflect")
    with pytest.raises(ValueError, match="n_original"):
        M.pitch_correlation(ok, ok, torch.zeros(2, dtype=torch.int32))              # a host tensor
    with pytest.raises(ValueError, match="tuning"):
        M.chroma_stft(ok, tuning=torch.zeros(3))
    if not torch.cuda.is_available():
        for fn in (M.chroma_stft, M.estimate_tuning, M.pitch_mean):
            with pytest.raises(RuntimeError, match="device tensors"):              # no CPU path
                fn(ok)
        for fn in (M.chroma_distance, M.chroma_similarity, M.pitch_correlation):
            with pytest.raises(RuntimeError, match="device tensors"):
                fn(ok, ok)


def test_transfer_and_score_takes_the_chroma_flag():
    import inspect
    from ast_amd.infer import StyleTransferSession
    assert inspect.signature(StyleTransferSession.transfer_and_score).parameters["chroma"].default is False
    sess = StyleTransferSession(torch.nn.Identity(), torch.nn.Identity(), use_graph=False)
    with pytest.raises(ValueError, match="cuda"):
        sess.transfer_and_score(torch.zeros(2, 90000), torch.zeros(2, 256), chroma=True)
