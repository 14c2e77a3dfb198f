"""Dataset screening without a GPU: what tests/test_gpu_curation.py relies on.  The float64 restatement (tests/curation_ref.py)
against plain loops on tiny inputs; the two identities the kernels are built on (a frame is four hop blocks; the mean of the DCT is
the DCT of the mean) to float64 rounding; the DCT against scipy; the mel grid at 44 100 Hz as ast_mel_table builds it; the margins
that let the GPU test demand exact equality of the integer results; the refusals of the C entries and the Python wrappers; and
DatasetReport's lines.  Parity with librosa's and pydub's own output stays unpinned: neither is available."""
import ctypes

import numpy as np
import pytest
import torch

import ast_amd
from ast_amd import _lib
from ast_amd import curation as Cu

import curation_ref as F
import mfcc_ref as MR

FAKE = 0x10000                                            # an aligned non-null pointer; nothing dereferences it


def _sample(x, i, pad_mode):
    n = len(x)
    if pad_mode == "reflect":
        i = -i if i < 0 else i
        i = 2 * (n - 1) - i if i >= n else i
        return x[i]
    return x[i] if 0 <= i < n else 0.0


@pytest.mark.parametrize("pad_mode,n", [("constant", 1), ("constant", 700), ("constant", 1536), ("reflect", 1025), ("reflect", 1600)])
def test_frame_rms_restatement_against_plain_loops(pad_mode, n):
    x = np.random.default_rng(n).standard_normal(n)
    got = F.frame_rms(x, pad_mode)
    assert len(got) == 1 + n // 512
    for t in range(len(got)):
        s = sum(_sample(x, i, pad_mode) ** 2 for i in range(512 * t - 1024, 512 * t + 1024))
        assert got[t] == pytest.approx((s / 2048) ** 0.5, rel=1e-13)
    assert F.silent_frames(x * 1e-3, pad_mode) == len(got) and F.silent_frames(x, pad_mode, threshold=0.0) == 0
    assert F.clip_rms(x) == pytest.approx((sum(v * v for v in x) / n) ** 0.5, rel=1e-13)


def test_window_and_gain_restatements_against_plain_loops():
    x = np.random.default_rng(3).standard_normal(1000) * np.repeat([1e-3, 1.0, 1e-2, 0.0, 5.7e-3], 200)
    # 100 ms at 2 000 Hz: windows of 200 samples
    lv = F.window_levels(x, 2000)
    assert len(lv) == 5 and len(F.window_levels(x[:999], 2000)) == 4 and len(F.window_levels(x[:199], 2000)) == 0
    for w in range(5):
        assert lv[w] == pytest.approx((sum(v * v for v in x[200 * w:200 * w + 200]) / 200) ** 0.5, rel=1e-13, abs=0)
    assert F.sound_windows(x, 2000).tolist() == [0, 1, 1, 0, int(20 * np.log10(lv[4]) > -45)]
    assert F.sound_ratio(x[:800], 2000) == 0.5 and F.sound_ratio(x[:199], 2000) == 0.0 and F.sound_ratio(np.zeros(900), 2000) == 0.0
    y = F.rms_normalize(x)
    assert F.clip_rms(y) == pytest.approx(0.07, rel=1e-13) and np.allclose(y * F.clip_rms(x), x * 0.07, rtol=1e-13, atol=0)
    z = np.zeros(7)
    assert F.rms_normalize(z) is z


@pytest.mark.parametrize("pad_mode", F.MODES)
def test_a_frame_is_four_hop_blocks(pad_mode):
    """the identity csrc/curation.hip is built on, to float64 rounding"""
    for x in F.clips(pad_mode):
        x = x.astype(np.float64)
        T = F.n_frames(len(x))
        p = F.padded(x, pad_mode)
        p = np.concatenate([p, np.zeros(512)])[:(T + 3) * 512]
        blocks = (p.reshape(-1, 512) ** 2).sum(axis=1)                                  # hop blocks -2 .. T
        four = np.sqrt((blocks[0:T] + blocks[1:T + 1] + blocks[2:T + 2] + blocks[3:T + 3]) / 2048)
        assert np.allclose(four, F.frame_rms(x, pad_mode), rtol=1e-13, atol=0)


def test_mean_of_the_dct_is_the_dct_of_the_mean():
    for sr in F.RATES:
        for b in (5, 9, F.MIX_ROW):
            x = F.clips("constant")[b]
            db = F.mel_db(x, sr)
            one = (MR.dct_matrix(13) @ db.mean(dim=1)).numpy()
            assert np.abs(one - F.mfcc_mean(x, sr)).max() <= 1e-12 * np.abs(one).max()
    # at 22 050 Hz the chain is the pinned MFCC restatement's
    x = F.clips("reflect")[9]
    assert torch.equal(F.mel_filters(22050), MR.mel_filters())
    assert np.array_equal(F.mfcc_frames(x, 22050, 13, 512, "reflect"), MR.mfcc(torch.from_numpy(x), 13, 512, "reflect").numpy())
    assert np.array_equal(F.mfcc_frames(x, 22050, 13, 256), MR.mfcc(torch.from_numpy(x), 13, 256).numpy())
    # silence: every dB value is -100, so coefficient 0 is -100 sqrt(128) and the others vanish
    c = F.mfcc_mean(np.zeros(5000, dtype=np.float32), 44100)
    assert c[0] == pytest.approx(-100 * 128 ** 0.5, rel=1e-12) and np.abs(c[1:]).max() < 1e-10


def test_dct_equals_scipy():
    fft = pytest.importorskip("scipy.fft")
    v = np.random.default_rng(0).standard_normal((128, 7))
    assert np.allclose(MR.dct_matrix(20).numpy() @ v, fft.dct(v, type=2, norm="ortho", axis=0)[:20], rtol=0, atol=1e-12)


def _dense(sample_rate):
    L = _lib.lib()
    words = (ctypes.c_int32 * L.ast_mel_table_words())()
    _lib.check(L.ast_mel_table(sample_rate, ctypes.addressof(words)), "ast_mel_table")
    w = np.array(words, dtype=np.int32)
    start, offs, wt = w[:128], w[128:257], w[257:].view(np.float32)
    W = np.zeros((128, 1025), dtype=np.float32)
    for i in range(128):
        W[i, start[i]:start[i] + offs[i + 1] - offs[i]] = wt[offs[i]:offs[i + 1]]
    return W


def test_mel_grid_at_44100_hz():
    """the table the kernels read at the clips' own rate is the documented filter bank rounded to float32"""
    for sr in (44100, 22050, 48000):
        W, ref = _dense(sr), F.mel_filters(sr).numpy()
        # float32 rounding; at the Nyquist bin the restatement's grid end is one rounding above sr / 2 and leaves 1e-17 there
        assert np.allclose(W, ref, rtol=6e-8, atol=1e-15), sr
        assert (W > 0).any(axis=1).all() and ((W > 0) == (ref > 1e-15)).all()
    f = MR.mel_frequencies(130, fmax=22050.0)
    assert f[0] == 0 and f[-1] == pytest.approx(22050.0, rel=1e-12) and np.all(np.diff(f) > 0)
    # Slaney: linear below 1 kHz, 200 / 3 Hz per mel
    step = MR.hz_to_mel(22050.0) / 129
    assert np.allclose(f[:10], np.arange(10) * step * 200 / 3, rtol=1e-12)


def test_constants_and_fixture_reach_every_case():
    lib = _lib.lib()
    assert lib.ast_frame_rms_tile_frames() == F.TILE and lib.ast_mfcc_mean_chunk_frames() == F.CHUNK
    assert (Cu.RMS_FRAME, Cu.RMS_HOP, Cu.SILENCE_RMS, Cu.SOUND_DB, Cu.TARGET_RMS) == (F.FRAME, F.HOP, F.SILENCE_RMS, F.SOUND_DB, F.TARGET_RMS)
    c = F.COUNTS["constant"]
    assert c[:6] == [1, 511, 512, 2047, 2048, 2049] and max(c) == F.N_MAX == fixture_width()
    assert F.n_frames(c[6]) == F.TILE and F.n_frames(c[7]) == F.TILE + 1 and c[8] == c[7] + 1                # the last frame of a tile, the next
    assert 2 * F.TILE < F.n_frames(F.N_MAX) <= 2 * F.TILE + 4                                                 # a little over two tiles
    assert min(F.COUNTS["reflect"]) == 1025 and F.n_frames(F.N_MAX) > 2 * F.CHUNK
    w = fixture()
    assert not w[F.ZERO_ROW].any() and w[:F.ZERO_ROW].any(axis=1).all()
    # the mixed clip: every one of the 16 loud / quiet mixes of four consecutive hop blocks occurs among its frames
    loud = [F.PATTERN[j % len(F.PATTERN)] for j in range(c[F.MIX_ROW] // 512)]
    assert {tuple(loud[j:j + 4]) for j in range(len(loud) - 3)} == {tuple(int(v) for v in f"{m:04b}") for m in range(16)}
    for pm in F.MODES:
        ref = F.references(pm)
        T = F.n_frames(F.COUNTS[pm][F.MIX_ROW])
        assert 0 < ref["silent"][F.MIX_ROW] < T and ref["silent"][F.ZERO_ROW] == F.n_frames(F.COUNTS[pm][F.ZERO_ROW])
        for sr in F.RATES:
            m = ref["sound"][sr][F.MIX_ROW]
            assert 0 < m.sum() < len(m) and ref["sound"][sr][F.ZERO_ROW].sum() == 0 and ref["sound"][sr][9].all()
    assert len(F.references("constant")["sound"][22050][0]) == 0 and len(F.references("constant")["sound"][44100][5]) == 0   # shorter than a window


def fixture():
    return F.fixture_waves().numpy()


def fixture_width():
    return F.fixture_waves().shape[1]


@pytest.mark.parametrize("pad_mode", F.MODES)
def test_fixture_margins_allow_exact_equality(pad_mode):
    """No fixture frame's RMS lies within 1e-4 relative of 0.005 and no window's level within 1e-3 dB of -45 in float64, so the GPU
    test compares the integer results exactly and excludes nothing."""
    near_rms, near_db = [], []
    for b, x in enumerate(F.clips(pad_mode)):
        r = F.frame_rms(x, pad_mode)
        near_rms.append(float(np.abs(r / F.SILENCE_RMS - 1).min()))
        for sr in F.RATES:
            lv = F.window_levels(x, sr)
            lv = lv[lv > 0]
            if len(lv):
                near_db.append(float(np.abs(F.level_db(lv) - F.SOUND_DB).min()))
    print(f"{pad_mode}: nearest frame RMS to the threshold {min(near_rms):.3g} relative, nearest window level {min(near_db):.3g} dB")
    assert min(near_rms) > 1e-4 and min(near_db) > 1e-3
    # the mixed clip's interior frames sit where the design puts them: quiet only and one loud block of four
    x = F.clips(pad_mode)[F.MIX_ROW]
    r = F.frame_rms(x, pad_mode)[2:-3]
    assert np.abs(r - 7.1e-4).min() < 2e-5 and np.abs(r - 7.1e-3).min() < 2e-4


@pytest.mark.parametrize("pad_mode", F.MODES)
def test_float32_twin_is_close_and_nonzero(pad_mode):
    """the floor the GPU bounds are 10 x of: a float32 error, not 0 and not large"""
    floor = F.f32_floor(pad_mode)
    print(f"{pad_mode}: float32 floors {floor}")
    for k, v in floor.items():
        assert 1e-9 < v < 5e-6, (k, v)
    # the twin's block layout reproduces the definition when carried out in float64
    x = F.clips(pad_mode)[9].astype(np.float64)
    bs, us = (t.astype(np.float64) for t in F.twin_blocks(x.astype(np.float32), pad_mode))
    assert us.sum() == pytest.approx((x ** 2).sum(), rel=1e-6)
    assert np.allclose(F.twin_frame_rms(x.astype(np.float32), pad_mode), F.frame_rms(x, pad_mode), rtol=1e-6, atol=0)


NEW = ("ast_frame_rms_tile_frames", "ast_mfcc_mean_chunk_frames", "ast_frame_rms_ws_floats", "ast_frame_rms_len", "ast_window_sound_len",
       "ast_mfcc_mean_ws_floats", "ast_mfcc_mean_len", "ast_gain_rows_len")


def test_entries_are_declared_and_exported():
    header = open(_lib.LIB_PATH.replace("audio-style-transfer_amd/ast_amd/libast_hip.so", "include/ast_hip.h")).read()
    for name in NEW:
        assert name in _lib.EXPORTS and name in _lib._SIGS and hasattr(_lib.lib(), name) and name + "(" in header
    for cite in ("silent_tracks_dataset.py:20-27", "dataset_tracks_analysis.py:27", "dataset_tracks_analysis.py:28-29", "dataset_variety.py:13-16",
                 "unifies_violin_datasets.py:25-30", "split_BachViolinDataset.py:24-30"):
        assert cite in header
    for name in ("frame_rms", "silence_ratio", "clip_rms", "sound_ratio", "sound_windows", "mfcc_mean", "rms_normalize", "screen", "DatasetReport"):
        assert getattr(ast_amd, name) is getattr(Cu, name)


def test_workspace_counts():
    lib = _lib.lib()
    run = lib.ast_mfcc_run_frames()
    big = 2 ** 31 - 1
    for B, n in ((12, F.N_MAX), (1, 1), (65535, big)):                                  # no 32-bit arithmetic on the way
        T = 1 + n // 512
        assert lib.ast_frame_rms_ws_floats(B, n) == 3 * B * -(-T // F.TILE)
        for hop in (256, 512):
            T = 1 + n // hop
            assert lib.ast_mfcc_mean_ws_floats(B, n, hop) == B * (T * 128 + -(-T // run)) + B * -(-T // F.CHUNK) * 128
            assert lib.ast_mfcc_mean_ws_floats(B, n, hop) == lib.ast_mfcc_ws_floats(B, n, hop) + B * -(-T // F.CHUNK) * 128
    assert lib.ast_frame_rms_ws_floats(0, 5) == 0 and lib.ast_frame_rms_ws_floats(3, 0) == 0
    assert lib.ast_mfcc_mean_ws_floats(3, 5, 128) == 0 and lib.ast_mfcc_mean_ws_floats(-1, 5, 512) == 0


def _refused(rc, entry, needle):
    err = _lib.lib().ast_last_error()
    assert rc == -1 and entry in err and needle in err, (rc, err)


ROWS = (dict(w=None), b"null"), (dict(B=0), b"bad shape"), (dict(B=65536), b"bad shape"), (dict(n=0), b"bad shape"), (dict(n=-4), b"bad shape"), \
       (dict(n=2 ** 31 - 4096), b"too long")


def test_entries_refuse_bad_arguments():
    """every new entry returns -1 with its message set before any launch: nothing here is a device pointer"""
    lib = _lib.lib()
    need = lib.ast_frame_rms_ws_floats(4, 12000)

    def rms(**kw):
        a = dict(w=FAKE, B=4, n=12000, ns=FAKE, thr=0.005, pad=0, ws=FAKE, wsn=need, rms=FAKE, nf=FAKE, sil=FAKE, ratio=FAKE, level=FAKE, sumsq=None)
        a.update(kw)
        return lib.ast_frame_rms_len(a["w"], a["B"], a["n"], a["ns"], a["thr"], a["pad"], a["ws"], a["wsn"], a["rms"], a["nf"], a["sil"], a["ratio"],
                                     a["level"], a["sumsq"], None)

    for kw, needle in ROWS + ((dict(rms=None), b"null"), (dict(nf=None), b"null"), (dict(sil=None), b"null"), (dict(ratio=None), b"null"),
                              (dict(level=None), b"null"), (dict(pad=2), b"pad_mode"), (dict(pad=-1), b"pad_mode"),
                              (dict(pad=1, n=1024), b"reflect"), (dict(ws=None), b"workspace"), (dict(wsn=need - 1), b"workspace"),
                              (dict(wsn=-1), b"workspace"), (dict(ws=FAKE + 4), b"aligned")):
        _refused(rms(**kw), b"ast_frame_rms_len", needle)

    def sound(**kw):
        a = dict(w=FAKE, B=4, n=12000, ns=FAKE, win=2205, thr=-45.0, mask=FAKE, ratio=FAKE)
        a.update(kw)
        return lib.ast_window_sound_len(a["w"], a["B"], a["n"], a["ns"], a["win"], a["thr"], a["mask"], a["ratio"], None)

    for kw, needle in ROWS + ((dict(ratio=None), b"null"), (dict(mask=None), b"null"), (dict(win=0), b"window"), (dict(win=-2205), b"window")):
        _refused(sound(**kw), b"ast_window_sound_len", needle)

    need = lib.ast_mfcc_mean_ws_floats(4, 12000, 512)

    def mean(**kw):
        a = dict(w=FAKE, B=4, n=12000, ns=FAKE, k=13, hop=512, pad=0, mel=FAKE, ws=FAKE, wsn=need, out=FAKE)
        a.update(kw)
        return lib.ast_mfcc_mean_len(a["w"], a["B"], a["n"], a["ns"], a["k"], a["hop"], a["pad"], a["mel"], a["ws"], a["wsn"], a["out"], None)

    for kw, needle in ROWS + ((dict(out=None), b"null"), (dict(mel=None), b"mel table"), (dict(k=0), b"n_mfcc"), (dict(k=21), b"n_mfcc"),
                              (dict(hop=128), b"hop"), (dict(hop=1024), b"hop"), (dict(pad=2), b"pad_mode"), (dict(pad=1, n=1024), b"reflect"),
                              (dict(ws=None), b"workspace"), (dict(wsn=need - 1), b"workspace"),
                              (dict(hop=256, wsn=lib.ast_mfcc_mean_ws_floats(4, 12000, 256) - 1), b"workspace")):
        _refused(mean(**kw), b"ast_mfcc_mean_len", needle)

    def gain(**kw):
        a = dict(w=FAKE, B=4, n=12000, ns=FAKE, ss=FAKE, target=0.07, out=FAKE)
        a.update(kw)
        return lib.ast_gain_rows_len(a["w"], a["B"], a["n"], a["ns"], a["ss"], a["target"], a["out"], None)

    for kw, needle in ROWS + ((dict(ss=None), b"null"), (dict(out=None), b"null"), (dict(target=0.0), b"target"), (dict(target=-1.0), b"target"),
                              (dict(target=float("nan")), b"target"), (dict(target=float("inf")), b"target")):
        _refused(gain(**kw), b"ast_gain_rows_len", needle)


def test_python_wrappers_refuse_bad_inputs():
    ok = torch.zeros(2, 3000)
    single = (Cu.frame_rms, Cu.silence_ratio, Cu.clip_rms, Cu.sound_ratio, Cu.sound_windows, Cu.mfcc_mean, Cu.rms_normalize, Cu.screen)
    for fn in single:
        for bad in (ok.double(), torch.zeros(2, 0), torch.zeros(2, 3, 3000), np.zeros((2, 3000), dtype=np.float32)):
            with pytest.raises(ValueError):
                fn(bad)
        with pytest.raises(ValueError, match="n_samples"):
            fn(ok, torch.zeros(2, dtype=torch.int64))
        with pytest.raises(RuntimeError, match="device tensors"):                     # a host tensor never reaches a kernel
            fn(ok)
    for fn in (Cu.frame_rms, Cu.silence_ratio, Cu.mfcc_mean, Cu.screen):
        with pytest.raises(ValueError, match="pad_mode"):
            fn(ok, pad_mode="edge")
        with pytest.raises(ValueError, match="1025"):
            fn(torch.zeros(2, 1024), pad_mode="reflect")
    for fn in (Cu.mfcc_mean, Cu.screen):
        for kw in (dict(n_mfcc=0), dict(n_mfcc=21), dict(n_mfcc=13.0), dict(hop_length=128), dict(sample_rate=0), dict(sample_rate=22050.0)):
            with pytest.raises(ValueError):
                fn(ok, **kw)
    for fn in (Cu.sound_ratio, Cu.sound_windows, Cu.screen):
        for kw in (dict(sample_rate=0), dict(frame_ms=0), dict(sample_rate=5, frame_ms=100)):
            with pytest.raises(ValueError):
                fn(ok, **kw)
    for bad in (0, -0.07, float("inf"), float("nan"), "0.07", True):
        with pytest.raises(ValueError, match="target_rms"):
            Cu.rms_normalize(ok, target_rms=bad)
    with pytest.raises(ValueError):
        Cu.screen(torch.zeros(2, 2, 3000, dtype=torch.float64))


def test_dataset_report_reproduces_the_scripts_lines():
    names = ["b.wav", "a.mp3", "c.wav"]
    res = dict(rms_level=torch.tensor([0.05, 0.1234, 0.0]), silence_ratio=torch.tensor([0.3, 0.29, 1.0]), sound_ratio=torch.tensor([0.6, 0.59, 0.0]),
               mfcc_mean=torch.tensor([[-300.0] + [1.0] * 12, [-250.5] + [2.0] * 12, [-1131.37] + [0.0] * 12]), n_frames=torch.tensor([44, 87, 44]))
    rep = Cu.DatasetReport()
    rep.add(names[:2], {k: v[:2] for k, v in res.items()}, torch.tensor([22050, 44100], dtype=torch.int32), 22050)
    rep.add(names[2:], {k: v[2:] for k, v in res.items()}, [22050], [44100])
    # silent_tracks_dataset.py:14-27: sorted file order, ratio >= 0.3
    assert [f for f, _ in rep.flagged()] == ["b.wav", "c.wav"] and rep.flagged()[0][1] == pytest.approx(0.3, rel=1e-6)
    assert rep.mostly_sound() == {"b.wav": True, "a.mp3": False, "c.wav": False}
    # dataset_tracks_analysis.py:48-54, the same format strings on the same lists
    stats = dict(filenames=names, durations=[1.0, 2.0, 0.5], rms_levels=res["rms_level"].double().tolist(), sample_rates=[22050, 22050, 44100],
                 mfcc_means=res["mfcc_mean"].double().numpy())
    want = ["\nDataset 1", f"• Files analyzed: {len(stats['filenames'])}", f"• Average duration: {np.mean(stats['durations']):.2f} sec",
            f"• Average RMS: {np.mean(stats['rms_levels']):.4f}", f"• Unique sample rates: {set(stats['sample_rates'])}",
            f"• Global average MFCC (first coefficient).: {np.mean([m[0] for m in stats['mfcc_means']]):.2f}"]
    assert rep.summary("Dataset 1") == "\n".join(want)
    with pytest.raises(ValueError):
        Cu.DatasetReport().summary("empty")
    with pytest.raises(ValueError):
        rep.add(names, res, [1, 2], 22050)
