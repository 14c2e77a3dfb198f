"""Onsets and self-similarity without a GPU: what tests/test_gpu_onset.py relies on.  The F1 formula against
sklearn.metrics.f1_score on the reference's construction; the restated neighbour rule against sklearn's NearestNeighbors; the
margins that let the GPU test demand exact equality of the discrete outputs; seeded mistakes in the restatement; and the refusals
of the C entries and the Python wrappers.  Parity with librosa's own output stays unpinned: librosa is not available."""
import inspect

import numpy as np
import pytest
import torch

import ast_amd
from ast_amd import _lib
from ast_amd import metrics as M

import onset_ref as F

FAKE = 0x10000                                            # an aligned non-null pointer; nothing dereferences it
MODES = ["constant", "reflect"]


def test_window_sizes_are_derived():
    src = inspect.getsource(F)
    assert "0.03 * SR // HOP" in src and "0.10 * SR // HOP" in src and "math.ceil(math.sqrt(" in src
    assert (F.PRE_MAX, F.POST_MAX, F.PRE_AVG, F.POST_AVG, F.WAIT, F.SHIFT, F.K, F.NN) == (1, 1, 4, 5, 1, 3, 10, 12)


def test_f1_formula_equals_sklearn_for_any_total_frames():
    """total_frames (evaluation_reconstruction.py:70) only sizes the arrays handed to f1_score"""
    gen = np.random.default_rng(5)
    cases = [([], []), ([], [3]), ([4, 9], []), ([2, 7, 11], [2, 7, 11]), ([2, 7, 11], [2, 8, 11]), ([1], [5, 6])]
    cases += [(sorted(gen.choice(40, 7, replace=False)), sorted(gen.choice(40, 5, replace=False))) for _ in range(5)]
    for o, g in cases:
        top = max(list(o) + list(g), default=0) + 1
        O, G = np.zeros(top, dtype=bool), np.zeros(top, dtype=bool)
        O[list(o)], G[list(g)] = True, True
        want = F.f1_formula(O, G)
        for total in (top, top + 1, top + 37, 1000):
            assert abs(F.f1_reference(list(o), list(g), total) - want) < 1e-15, (o, g, total)


@pytest.mark.parametrize("pad_mode", MODES)
def test_neighbour_rule_equals_sklearn(pad_mode):
    ref = F.references(pad_mode)
    for w, b in F.ranked_clips(pad_mode):
        c = ref[w][b]["coef"]
        assert np.array_equal(F.recurrence_sklearn(c), ref[w][b]["R"]), (w, b)
        assert np.array_equal(F.neighbour_rule(np.sqrt(ref[w][b]["d2"])), ref[w][b]["R"])             # squared or not: the same order
    # exact zeros: duplicated points are at distance 0 of each other, and the sparse graph loses those links
    gen = np.random.default_rng(6)
    c = gen.standard_normal((20, 9))
    c[7], c[12], c[13] = c[3], c[3], c[5]
    D2 = F.distances2(c)
    R, S = F.neighbour_rule(D2), F.recurrence_sklearn(c)
    for j in range(20):                                    # duplicates tie for every other column, and sklearn promises no tie order:
        if j in (3, 7, 12, 5, 13):                         # the columns with zeros have no tie at the cut and agree entry by entry,
            assert np.array_equal(S[:, j], R[:, j]), j
        assert np.array_equal(np.sort(D2[S[:, j] == 1, j]), np.sort(D2[R[:, j] == 1, j])), j     # the others in the distances kept
    assert R[7, 3] == R[12, 3] == R[3, 7] == R[5, 13] == 0 and int(R[:, 3].sum()) == 10 and int(np.trace(R)) == 0


def test_silence_and_single_samples_have_no_margin():
    """why ranked_clips leaves them out: the issue expected silence's rows 1 .. 19 at distance exactly 0; in float64 they are
    rounding noise apart, and a one-sample clip's lie closer together than float32 resolves"""
    ref, tw = F.references("constant"), F.twin("constant")
    off = ~np.eye(19, dtype=bool)
    D = np.sqrt(ref[F.SILENT[0]][F.SILENT[1]]["d2"])
    assert 0 < D[1:, 1:][off].max() < 1e-8 * D.max()
    for w in ("orig", "gen"):                              # the float32 floor of these distances is as large as the distances
        D, D32 = np.sqrt(ref[w][3]["d2"])[1:, 1:][off], np.sqrt(tw[w][3]["d2"].astype(np.float64))[1:, 1:][off]
        assert float((np.abs(D32 - D) / D).max()) > 0.1, w
    c = ref[F.SILENT[0]][F.SILENT[1]]["coef"]
    assert abs(c[0, 0] + 100 * np.sqrt(128)) < 1e-9 and np.abs(c[1:]).max() < 1e-10


@pytest.mark.parametrize("pad_mode", MODES)
def test_fixture_margins_allow_exact_equality(pad_mode):
    """The float32 twin's error is the unit; every decision of the float64 restatement must lie 10 units from its threshold."""
    ref, tw = F.references(pad_mode), F.twin(pad_mode)
    for w in ("orig", "gen"):
        for b in range(F.B):
            r, t = ref[w][b], tw[w][b]
            assert np.array_equal(r["mask"], t["mask"]), (w, b)
            if not r["env"].any():
                assert not t["env"].any() and not r["mask"].any()
                continue
            err = float(np.abs(F.normalised(r["env"]) - F.normalised(t["env"]).astype(np.float64)).max())
            margins = []
            F.onset_detect(r["env"], margins)
            m_avg = min(m[1] for m in margins)
            m_max = min([m[0] for m in margins if m[2]] or [np.inf])                    # wherever the maximum condition decides
            print(f"{pad_mode} {w}{b}: envelope error {err:.2e}, margins {m_max:.2e} (maximum) {m_avg:.2e} (mean + delta)")
            assert 0 < err < 1e-5 and m_avg > 10 * err and m_max > 10 * err, (w, b, err, m_avg, m_max)
    for w, b in F.ranked_clips(pad_mode):
        r, t = ref[w][b], tw[w][b]
        assert np.array_equal(r["R"], t["R"]), (w, b)
        D, D32 = np.sqrt(r["d2"]), np.sqrt(t["d2"].astype(np.float64))
        off = ~np.eye(F.N_MFCC, dtype=bool)
        err = float((np.abs(D32 - D)[off] / D[off]).max())
        gaps = []
        for j in range(F.N_MFCC):
            d = np.sort(np.delete(D[:, j], j))
            assert d[0] > 0
            gaps.append((d[F.K] - d[F.K - 1]) / d[F.K])
        zero_gap = float(D[off].min() / D.max())
        print(f"{pad_mode} {w}{b}: distance error {err:.2e}, smallest 10th-to-11th gap {min(gaps):.2e}, smallest distance {zero_gap:.2e} of the largest")
        assert 0 < err < 1e-4 and min(gaps) > 10 * err and zero_gap > 10 * err, (w, b, err, min(gaps), zero_gap)
    assert ref["acc"] == tw["acc"]
    assert 0 < ref["acc"][0] < 1 and ref["acc"][2] == 0.0 and ref["acc"][3] == 1.0


def test_fixture_reaches_every_tile_case():
    tile, chunk = _lib.lib().ast_onset_tile_frames(), _lib.lib().ast_recurrence_chunk_frames()
    frames = sorted({F.n_frames(n) for pm in MODES for n in F.COUNTS[pm] + F.N_GENERATED[pm]})
    assert any(3 < T < tile for T in frames) and any(T > tile and T % tile for T in frames) and any(T > tile and T % tile == 0 for T in frames)
    assert any(T <= 3 for T in frames) and any(T > chunk and T % chunk for T in frames) and max(F.N_ORIG, F.N_GEN) <= 12000
    assert F.N_ORIG != F.N_GEN


def test_seeded_mistakes_change_a_score():
    pm = "constant"
    ref, cl = F.references(pm), F.clips(pm)
    a, g = F.fixture_waves()
    acc, ssd = ref["acc"], ref["ssd"]
    # counts ignored: the rows taken as full
    assert [F.onset_accuracy(a[b], g[b], pm) for b in range(F.B)] != acc
    assert [F.self_similarity_distance(a[b], g[b], pm) for b in range(F.B)] != ssd
    # clips not cut to the common length
    assert [F.onset_accuracy(x, y, pm, cut=False) for x, y in cl] != acc
    # the 3-frame shift dropped: every mask moves; both clips of a pair move alike, so an F1 changes only where an onset enters at
    # the cut end, which row 1 shows under reflect padding (1/3 -> 2/3)
    masks = [F.onset_detect(F.onset_strength(x, pm, shift=1)) for x, _ in cl]
    assert any(not np.array_equal(m, ref["orig"][b]["mask"]) for b, m in enumerate(masks))
    assert [F.onset_accuracy(x, y, "reflect", shift=1) for x, y in F.clips("reflect")] != F.references("reflect")["acc"]
    # the clamp taken from the batch maximum
    batch_max = max(float(F.MF.mel_db(x, F.HOP, pm).max()) for pair in cl for x in pair)
    env = [F.onset_strength(y, pm, clamp_max=batch_max) for _, y in cl]
    assert any(F.env_error(e, ref["gen"][b]["env"]) > 1e-3 for b, e in enumerate(env))
    assert [F.onset_accuracy(x, y, pm, clamp_max=batch_max) for x, y in cl] != acc
    # 12 neighbours kept instead of 10; R symmetrised
    assert [F.self_similarity_distance(x, y, pm, keep=F.NN) for x, y in cl] != ssd
    assert [F.self_similarity_distance(x, y, pm, sym=True) for x, y in cl] != ssd


def test_entries_are_declared_and_exported():
    for name in ("ast_onset_tile_frames", "ast_recurrence_chunk_frames", "ast_onset_strength_len", "ast_onset_detect_len",
                 "ast_onset_accuracy_len", "ast_recurrence_len", "ast_self_similarity_distance_len"):
        assert name in _lib.EXPORTS and name in _lib._SIGS and hasattr(_lib.lib(), name)
        if name.endswith("_len"):
            assert name[:-4] + "_ws_floats" in _lib._SIGS
    header = open(_lib.LIB_PATH.replace("audio-style-transfer_amd/ast_amd/libast_hip.so", "include/ast_hip.h")).read()
    for name in ("ast_onset_strength_len", "ast_onset_detect_len", "ast_onset_accuracy_len", "ast_recurrence_len",
                 "ast_self_similarity_distance_len"):
        assert name + "(" in header
    assert "evaluation_reconstruction.py:54-81" in header and "evaluation_style_transfer.py:121-133" in header
    for name in ("onset_strength", "onset_detect", "onset_accuracy", "recurrence_matrix", "self_similarity_distance"):
        assert getattr(ast_amd, name) is getattr(M, name)


def test_workspace_counts():
    lib = _lib.lib()
    run, tile, chunk = lib.ast_mfcc_run_frames(), lib.ast_onset_tile_frames(), lib.ast_recurrence_chunk_frames()

    def pass1(B, n):
        T = 1 + n // 512
        return B * (T * 128 + -(-T // run))

    def strength(B, n):
        return pass1(B, n) + 2 * B * -(-(1 + n // 512) // tile)

    def detect(B, n):
        return strength(B, n) + B * (1 + n // 512)

    def rec(B, n):
        T = 1 + n // 512
        return pass1(B, n) + B * 20 * T + B * -(-T // chunk) * 190

    big = 2 ** 31 - 1
    for B, n, m in ((4, 12000, 11000), (1, 1, 1), (65535, big, big)):                 # no 32-bit arithmetic on the way
        assert lib.ast_onset_strength_ws_floats(B, n) == strength(B, n)
        assert lib.ast_onset_detect_ws_floats(B, n) == detect(B, n)
        assert lib.ast_onset_accuracy_ws_floats(B, n, m) == B + detect(B, n) + detect(B, m) + B * (2 + n // 512 + m // 512)
        assert lib.ast_recurrence_ws_floats(B, n) == rec(B, n)
        assert lib.ast_self_similarity_distance_ws_floats(B, n, m) == rec(B, n) + rec(B, m) + 2 * B * 400
    assert lib.ast_onset_strength_ws_floats(0, 5) == 0 and lib.ast_onset_detect_ws_floats(3, 0) == 0 and lib.ast_recurrence_ws_floats(-1, 5) == 0
    assert lib.ast_onset_accuracy_ws_floats(3, 5, 0) == 0 and lib.ast_self_similarity_distance_ws_floats(3, -5, 5) == 0


def _refused(rc, entry, needle):
    err = _lib.lib().ast_last_error()
    assert rc != 0 and entry in err and needle in err, (rc, err)


ONE = (dict(w=None), b"null"), (dict(out=None), b"null"), (dict(mel=None), b"mel table"), (dict(B=0), b"bad shape"), \
      (dict(B=65536), b"bad shape"), (dict(n=0), b"bad shape"), (dict(pad=2), b"pad_mode"), (dict(pad=-1), b"pad_mode"), \
      (dict(pad=1, n=1024), b"reflect"), (dict(n=2 ** 31 - 4096), b"too long"), (dict(ws=None), b"workspace"), (dict(wsn=-1), b"workspace")
PAIR = (dict(a=None), b"null"), (dict(g=None), b"null"), (dict(out=None), b"null"), (dict(mel=None), b"mel table"), \
       (dict(B=0), b"bad shape"), (dict(B=65536), b"bad shape"), (dict(na=0), b"bad shape"), (dict(ng=-3), b"bad shape"), \
       (dict(pad=3), b"pad_mode"), (dict(pad=1, na=1024), b"reflect"), (dict(pad=1, ng=1024), b"reflect"), \
       (dict(ng=2 ** 31 - 4096), b"too long"), (dict(ws=None), b"workspace"), (dict(wsn=-1), b"workspace")


def test_entries_refuse_bad_arguments():
    """what ast_mfcc_len and ast_mfcc_distance_len refuse, before any launch"""
    lib = _lib.lib()
    for entry in ("ast_onset_strength", "ast_onset_detect", "ast_recurrence"):
        need = getattr(lib, entry + "_ws_floats")(4, 12000)

        def one(**kw):
            a = dict(w=FAKE, B=4, n=12000, ns=FAKE, pad=0, mel=FAKE, ws=FAKE, wsn=need, out=FAKE)
            a.update(kw)
            args = [a["w"], a["B"], a["n"], a["ns"], a["pad"], a["mel"], a["ws"], a["wsn"], a["out"]]
            return getattr(lib, entry + "_len")(*args, *([None] if entry == "ast_recurrence" else []), None)

        for kw, needle in ONE + ((dict(wsn=need - 1), b"workspace"),):
            _refused(one(**kw), (entry + "_len").encode(), needle)
    for entry in ("ast_onset_accuracy", "ast_self_similarity_distance"):
        need = getattr(lib, entry + "_ws_floats")(4, 12000, 11000)

        def pair(**kw):
            a = dict(a=FAKE, na=12000, g=FAKE, ng=11000, B=4, la=FAKE, lg=FAKE, pad=0, mel=FAKE, ws=FAKE, wsn=need, out=FAKE)
            a.update(kw)
            return getattr(lib, entry + "_len")(a["a"], a["na"], a["g"], a["ng"], a["B"], a["la"], a["lg"], a["pad"], a["mel"], a["ws"],
                                                a["wsn"], a["out"], None)

        for kw, needle in PAIR + ((dict(wsn=need - 1), b"workspace"),):
            _refused(pair(**kw), (entry + "_len").encode(), needle)


def test_python_wrappers_refuse_bad_inputs():
    ok = torch.zeros(2, 3000)
    singles = (M.onset_strength, M.onset_detect, M.recurrence_matrix, M.recurrence_debug)
    pairs = (M.onset_accuracy, M.self_similarity_distance)
    for fn in singles:
        for bad in (ok.double(), torch.zeros(2, 2, 3000), torch.zeros(2, 0), np.zeros((2, 3000), dtype=np.float32)):
            with pytest.raises(ValueError):
                fn(bad)
        with pytest.raises(ValueError, match="pad_mode"):
            fn(ok, pad_mode="edge")
        with pytest.raises(ValueError, match="1025"):
            fn(torch.zeros(2, 1024), pad_mode="reflect")
        for bad in (torch.zeros(2), torch.zeros(2, dtype=torch.int64), torch.zeros(3, dtype=torch.int32), [3000, 3000],
                    torch.zeros(2, dtype=torch.int32)):                                # the last: a host tensor
            with pytest.raises(ValueError, match="n_samples"):
                fn(ok, bad)
    for fn in pairs:
        for args in ((ok, ok[0]), (ok, torch.zeros(3, 3000)), (ok.long(), ok)):
            with pytest.raises(ValueError):
                fn(*args)
        with pytest.raises(ValueError, match="pad_mode"):
            fn(ok, ok, pad_mode="edge")
        with pytest.raises(ValueError, match="1025"):
            fn(ok, torch.zeros(2, 1024), pad_mode="reflect")
        with pytest.raises(ValueError, match="n_"):
            fn(ok, ok, None, torch.zeros(2, dtype=torch.int32))
    if not torch.cuda.is_available():
        for fn in singles:
            with pytest.raises(RuntimeError, match="device tensors"):                  # no CPU path
                fn(ok)
        for fn in pairs:
            with pytest.raises(RuntimeError, match="device tensors"):
                fn(ok, ok)


def test_transfer_and_score_takes_the_two_flags():
    from ast_amd.infer import StyleTransferSession
    params = inspect.signature(StyleTransferSession.transfer_and_score).parameters
    assert params["onsets"].default is False and params["self_similarity"].default is False
    sess = StyleTransferSession(torch.nn.Identity(), torch.nn.Identity(), use_graph=False)
    with pytest.raises(ValueError, match="cuda"):                                      # transfer's own checks still come first
        sess.transfer_and_score(torch.zeros(2, 90000), torch.zeros(2, 256), onsets=True, self_similarity=True)
