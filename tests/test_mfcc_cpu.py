"""MFCC without a GPU: what the float64 restatement (tests/mfcc_ref.py) that tests/test_gpu_mfcc.py checks the kernels against
is pinned to -- the mel grid to the values printed in librosa.mel_frequencies' docstring, the DCT to scipy.fft.dct, the library's
host-built filter table to the restated filter bank --, that the fixture reaches both clamps, that seeded mistakes move a
distance by far more than the tolerance, and that the C entries and the Python wrappers refuse bad calls before any launch.
Parity with librosa's own output stays unpinned: librosa is not available."""
import ctypes

import numpy as np
import pytest
import scipy.fft
import torch

import ast_amd
from ast_amd import _lib
from ast_amd import metrics as M

import mfcc_ref as F

FAKE = 0x10000                                            # an aligned non-null pointer; nothing dereferences it


def test_mel_grid_equals_the_docstring_values():
    """librosa.mel_frequencies(n_mels=40) prints 0, 85.317, 170.635, ..., 1024.856, 1119.114, ..., 11025 (fmin 0, fmax 11025)"""
    f = F.mel_frequencies(40)
    for i, want in ((0, 0.0), (1, 85.317), (2, 170.635), (12, 1024.856), (13, 1119.114), (39, 11025.0)):
        assert abs(f[i] - want) < 1e-3, (i, f[i])
    assert np.all(np.diff(f) > 0)
    # the two branches of the scale meet at 1 kHz = 15 mel, and the inverse inverts
    assert abs(float(F.hz_to_mel(1000.0)) - 15.0) < 1e-12 and abs(float(F.hz_to_mel(999.999)) - 14.999985) < 1e-9
    g = np.array([0.0, 440.0, 999.0, 1000.0, 1001.0, 5000.0, 11025.0])
    assert np.abs(F.mel_to_hz(F.hz_to_mel(g)) - g).max() < 1e-9


def test_filter_bank_properties():
    W = F.mel_filters().numpy()
    nz = W > 0
    assert W.shape == (128, 1025) and int(nz.sum(axis=0).max()) == 2             # a bin feeds at most 2 filters
    spans = nz.sum(axis=1)
    assert int(spans.min()) == 4 and int(spans.max()) == 53                       # no filter is empty
    for i in range(128):                                                          # a filter's bins are consecutive
        k = np.flatnonzero(nz[i])
        assert k[-1] - k[0] + 1 == len(k)
    # Slaney normalisation: a triangle of height 2 / width, sampled every 11025 / 1024 Hz, has area about 1
    area = W.sum(axis=1) * (11025 / 1024)
    assert np.abs(area[20:] - 1).max() < 0.05 and np.abs(area - 1).max() < 0.25


def test_host_table_equals_the_restated_filter_bank():
    """ast_mel_table (C, double, no device) against mfcc_ref.mel_filters: the same support, weights equal to float32 rounding"""
    lib = _lib.lib()
    n = lib.ast_mel_table_words()
    assert n == 2 * 128 + 1 + 2 * 1025
    words = (ctypes.c_int32 * n)()
    assert lib.ast_mel_table(22050, ctypes.addressof(words)) == 0
    w = np.array(words, dtype=np.int32)
    start, offs, wt = w[:128], w[128:257], w[257:].view(np.float32)
    assert offs[0] == 0 and np.all(np.diff(offs) >= 4) and offs[128] <= 2 * 1025 and np.all(wt[offs[128]:] == 0)
    dense = np.zeros((128, 1025))
    for i in range(128):
        dense[i, start[i]:start[i] + offs[i + 1] - offs[i]] = wt[offs[i]:offs[i + 1]]
    W = F.mel_filters().numpy()
    assert np.array_equal(dense > 0, W > 0)
    assert np.abs(dense - W).max() <= 2.0 ** -24 * W.max()
    # other rates fill a table too; a null pointer and a rate below 1 Hz are refused with a message
    assert lib.ast_mel_table(48000, ctypes.addressof(words)) == 0 and lib.ast_mel_table(8000, ctypes.addressof(words)) == 0
    assert lib.ast_mel_table(22050, None) != 0 and b"ast_mel_table" in lib.ast_last_error()
    assert lib.ast_mel_table(0, ctypes.addressof(words)) != 0 and b"sample rate" in lib.ast_last_error()


def test_dct_equals_scipy():
    gen = torch.Generator().manual_seed(3)
    db = torch.randn(128, 37, generator=gen, dtype=torch.float64) * 40
    for n_mfcc in (1, 13, 20, 128):
        want = scipy.fft.dct(db.numpy(), type=2, norm="ortho", axis=0)[:n_mfcc]
        assert np.abs((F.dct_matrix(n_mfcc) @ db).numpy() - want).max() < 1e-11
    x = torch.randn(5000, generator=gen)
    want = scipy.fft.dct(torch.maximum(F.mel_db(x, 512), F.mel_db(x, 512).max() - 80).numpy(), type=2, norm="ortho", axis=0)[:20]
    assert np.abs(F.mfcc(x).numpy() - want).max() < 1e-11


def test_fixture_reaches_both_clamps():
    for hop in (256, 512):
        for b, pair in enumerate(F.clips("constant")):
            for x in pair:
                db = F.mel_db(x, hop)
                top, amin = float((db < db.max() - 80).double().mean()), float((db <= -100).double().mean())
                if b == 1:                                  # the sine over 1e-5 noise: most values sit on the top_db clamp
                    assert 0.75 < top < 0.9 and amin == 0.0, (hop, top, amin)
                elif b == 2:                                # noise x 1.2e-6: most values on the 1e-10 floor, the rest above it
                    assert 0.5 < amin < 0.85 and top == 0.0, (hop, top, amin)
                else:
                    assert top == 0.0 and amin == 0.0, (hop, b, top, amin)


def test_seeded_mistakes_move_a_distance_by_more_than_100_bounds():
    """By the float64 restatement alone, in units of the GPU test's bound on a distance (10 x the float32 floor, relative to the
    pair's peak |coefficient|; the bound is 3.4e-6 here and moves a little with the host's FFT library).  Measured at (13, 256) / (20, 512):
        no top_db clamp:             row 1   153.58 -> 294.28, 100 000 x  /  164.36 -> 298.88, 96 000 x
        counts ignored (full rows):  row 3   291.13 -> 14.32,  560 000 x  /  291.94 -> 18.17,  550 000 x   (row 1: 1 300 x / 1 700 x)
        HTK instead of Slaney mel:   row 3   291.13 -> 293.19,   4 200 x  /  291.94 -> 293.71,   3 600 x   (rows 0 and 2: 190 x / 330 x and 116 x / 149 x)
        clamp by the maximum over the whole batch instead of the clip's own: row 2   7.25 -> 0, 6.93 -> 0: 1 900 x / 1 800 x
    The clamp by the OTHER CLIP OF THE PAIR moves row 1 by 6 x / 30 x the bound and no row by 100 x: the two sines have nearly
    the same maximum, and on no other row is the top_db clamp active.  That is above the bound, so a kernel that swaps the two
    maxima fails the GPU comparison, but the fixture the issue prescribes cannot show it with a margin of 100; asserted is what
    the comparison needs, more than 1 x the bound, and the 100 x for the batch-wide form of the same mistake."""
    pm = "constant"
    bound = F.bounds(pm)["dist"]
    assert 0 < bound < 1e-5
    a, g = F.fixture_waves()
    for n_mfcc, hop in F.SETTINGS:
        ref, cl = F.references(pm, n_mfcc, hop), F.clips(pm)
        batch_max = max(float(F.mel_db(x, hop).max()) for pair in cl for x in pair)

        def moved(b, value):
            return abs(float(value) - float(ref["dist"][b])) / ref["peak_pair"][b] / bound

        x, y = cl[1]
        no_top = moved(1, F.mfcc_distance(y, x, n_mfcc, hop, pm, top_db=None))
        swapped = moved(1, F.mfcc_distance(y, x, n_mfcc, hop, pm, swap_max=True))
        full = [moved(b, F.mfcc_distance(g[b], a[b], n_mfcc, hop, pm)) for b in (1, 3)]
        htk = [moved(b, F.mfcc_distance(cl[b][1], cl[b][0], n_mfcc, hop, pm, htk=True)) for b in range(F.B)]
        x, y = cl[2]
        bm = torch.tensor(batch_max, dtype=torch.float64)
        mx, my = F.mfcc(x, n_mfcc, hop, pm, clamp_max=bm), F.mfcc(y, n_mfcc, hop, pm, clamp_max=bm)
        T = min(mx.shape[1], my.shape[1])
        batch = moved(2, ((my[:, :T] - mx[:, :T]) ** 2).sum(dim=0).sqrt().mean())
        print(f"({n_mfcc}, {hop}), in bounds of {bound:.3g}: no top_db {no_top:.0f}, counts ignored {full}, HTK {htk}, "
              f"batch-wide maximum {batch:.0f}, the pair's maxima swapped {swapped:.1f}")
        assert no_top > 100 and max(full) > 100 and max(htk) > 100 and batch > 100     # each mistake on the row named above
        assert swapped > 1


def test_entries_are_declared_and_exported():
    for name in ("ast_mel_table_words", "ast_mel_table", "ast_mfcc_run_frames", "ast_mfcc_ws_floats", "ast_mfcc_len",
                 "ast_mfcc_distance_ws_floats", "ast_mfcc_distance_len"):
        assert name in _lib.EXPORTS and name in _lib._SIGS and hasattr(_lib.lib(), name)
    assert ast_amd.mfcc is M.mfcc and ast_amd.mfcc_distance is M.mfcc_distance


def test_workspace_counts():
    lib = _lib.lib()
    run = lib.ast_mfcc_run_frames()
    assert run >= 1

    def one(B, n, hop):
        T = 1 + n // hop
        return B * (T * 128 + -(-T // run))

    for hop in (256, 512):
        assert lib.ast_mfcc_ws_floats(4, 40000, hop) == one(4, 40000, hop)
        assert lib.ast_mfcc_distance_ws_floats(4, 40000, 30000, hop) == one(4, 40000, hop) + one(4, 30000, hop) + 4 * (1 + 30000 // hop)
    assert lib.ast_mfcc_ws_floats(0, 5, 256) == 0 and lib.ast_mfcc_ws_floats(3, 0, 256) == 0 and lib.ast_mfcc_ws_floats(3, 5, 300) == 0
    assert lib.ast_mfcc_distance_ws_floats(3, 5, 0, 512) == 0 and lib.ast_mfcc_distance_ws_floats(3, 5, 5, 0) == 0
    big = 2 ** 31 - 1
    assert lib.ast_mfcc_ws_floats(65535, big, 256) == one(65535, big, 256)         # no 32-bit arithmetic on the way


def _refused(rc, entry, needle):
    err = _lib.lib().ast_last_error()
    assert rc != 0 and entry in err and needle in err, (rc, err)


def test_entries_refuse_bad_arguments():
    lib = _lib.lib()
    need = lib.ast_mfcc_ws_floats(4, 40000, 512)

    def mfcc(**kw):
        a = dict(w=FAKE, B=4, n=40000, ns=FAKE, k=20, hop=512, pad=0, mel=FAKE, ws=FAKE, wsn=need, out=FAKE)
        a.update(kw)
        return lib.ast_mfcc_len(a["w"], a["B"], a["n"], a["ns"], a["k"], a["hop"], a["pad"], a["mel"], a["ws"], a["wsn"], a["out"], None)

    for kw, needle in ((dict(w=None), b"null"), (dict(out=None), b"null"), (dict(mel=None), b"mel table"), (dict(B=0), b"bad shape"),
                       (dict(B=65536), b"bad shape"), (dict(n=0), b"bad shape"), (dict(k=0), b"n_mfcc"), (dict(k=129), b"n_mfcc"),
                       (dict(hop=128), b"hop"), (dict(hop=0), b"hop"), (dict(hop=1024), b"hop"), (dict(pad=2), b"pad_mode"),
                       (dict(pad=-1), b"pad_mode"), (dict(pad=1, n=1024), b"reflect"), (dict(n=2 ** 31 - 4096), b"too long"),
                       (dict(ws=None), b"workspace"), (dict(wsn=need - 1), b"workspace"), (dict(hop=256), b"workspace")):
        _refused(mfcc(**kw), b"ast_mfcc_len", needle)

    need = lib.ast_mfcc_distance_ws_floats(4, 40000, 30000, 256)

    def dist(**kw):
        a = dict(g=FAKE, ng=40000, r=FAKE, nr=30000, B=4, lg=FAKE, lr=FAKE, k=13, hop=256, pad=0, mel=FAKE, ws=FAKE, wsn=need, out=FAKE)
        a.update(kw)
        return lib.ast_mfcc_distance_len(a["g"], a["ng"], a["r"], a["nr"], a["B"], a["lg"], a["lr"], a["k"], a["hop"], a["pad"], a["mel"],
                                         a["ws"], a["wsn"], a["out"], None)

    for kw, needle in ((dict(g=None), b"null"), (dict(r=None), b"null"), (dict(out=None), b"null"), (dict(mel=None), b"mel table"),
                       (dict(B=0), b"bad shape"), (dict(B=65536), b"bad shape"), (dict(ng=0), b"bad shape"), (dict(nr=-3), b"bad shape"),
                       (dict(k=0), b"n_mfcc"), (dict(k=129), b"n_mfcc"), (dict(hop=100), b"hop"), (dict(pad=3), b"pad_mode"),
                       (dict(pad=1, ng=1024), b"reflect"), (dict(pad=1, nr=1024), b"reflect"), (dict(nr=2 ** 31 - 4096), b"too long"),
                       (dict(ws=None), b"workspace"), (dict(wsn=need - 1), b"workspace"), (dict(wsn=-1), b"workspace")):
        _refused(dist(**kw), b"ast_mfcc_distance_len", needle)


def test_python_wrappers_refuse_bad_inputs():
    ok = torch.zeros(2, 3000)
    for fn, args in ((M.mfcc, (ok.double(),)), (M.mfcc, (torch.zeros(2, 2, 3000),)), (M.mfcc, (torch.zeros(2, 0),)),
                     (M.mfcc, (np.zeros((2, 3000), dtype=np.float32),)), (M.mfcc_distance, (ok, ok[0])),
                     (M.mfcc_distance, (ok, torch.zeros(3, 3000))), (M.mfcc_distance, (ok.long(), ok))):
        with pytest.raises(ValueError):
            fn(*args)
    for kw in (dict(n_mfcc=0), dict(n_mfcc=129), dict(n_mfcc=True), dict(n_mfcc=13.0), dict(hop_length=128), dict(hop_length=1024)):
        with pytest.raises(ValueError, match="n_mfcc|hop_length"):
            M.mfcc(ok, **kw)
        with pytest.raises(ValueError, match="n_mfcc|hop_length"):
            M.mfcc_distance(ok, ok, **kw)
    with pytest.raises(ValueError, match="pad_mode"):
        M.mfcc(ok, pad_mode="edge")
    with pytest.raises(ValueError, match="1025"):
        M.mfcc(torch.zeros(2, 1024), pad_mode="reflect")
    with pytest.raises(ValueError, match="1025"):
        M.mfcc_distance(ok, torch.zeros(2, 1024), pad_mode="reflect")
    for bad in (torch.zeros(2), torch.zeros(2, dtype=torch.int64), torch.zeros(3, dtype=torch.int32), [3000, 3000]):
        with pytest.raises(ValueError, match="n_samples"):
            M.mfcc(ok, bad)
    with pytest.raises(ValueError, match="n_reference"):
        M.mfcc_distance(ok, ok, None, torch.zeros(2, dtype=torch.int32))           # a host tensor
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="device tensors"):                  # no CPU path
            M.mfcc(ok)
        with pytest.raises(RuntimeError, match="device tensors"):
            M.mfcc_distance(ok, ok)


def test_transfer_and_score_takes_the_mfcc_flag():
    """the default is off, and transfer's own argument checks still come first"""
    import inspect
    from ast_amd.infer import StyleTransferSession
    assert inspect.signature(StyleTransferSession.transfer_and_score).parameters["mfcc"].default is False
    sess = StyleTransferSession(torch.nn.Identity(), torch.nn.Identity(), use_graph=False)
    with pytest.raises(ValueError, match="cuda"):
        sess.transfer_and_score(torch.zeros(2, 90000), torch.zeros(2, 256), mfcc=True)
