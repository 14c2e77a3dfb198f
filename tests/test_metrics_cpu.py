"""Spectrogram metrics without a GPU: the float64 restatement that tests/test_gpu_metrics.py checks the kernels against
(tests/metrics_ref.py) equals torch.stft followed by the reference's formulas; the host argument checks of the C entries refuse
every bad call before any launch; the Python wrappers raise ValueError for bad dtypes, shapes and pad modes; and the fixture's
counts and pad modes move the metrics by far more than the tolerance, so a kernel that ignores either cannot pass."""
import numpy as np
import pytest
import torch

import ast_amd
from ast_amd import _lib
from ast_amd import metrics as M

import metrics_ref as R

FAKE = 0x10000                                            # an aligned non-null pointer; nothing dereferences it


def _torch_mag(x, n_fft, hop, pad_mode):
    x = torch.as_tensor(x, dtype=torch.float64)
    return torch.stft(x, n_fft, hop_length=hop, window=torch.hann_window(n_fft, dtype=torch.float64), center=True, pad_mode=pad_mode,
                      return_complex=True).abs()


@pytest.mark.parametrize("pad_mode", ["constant", "reflect"])
def test_restatement_equals_torch_stft(pad_mode):
    gen = torch.Generator().manual_seed(17)
    for n_fft, hop in ((R.MSE_N_FFT, R.MSE_HOP), (R.BAND_N_FFT, R.BAND_HOP)):
        for n in (n_fft // 2 + 1, n_fft, 3 * hop, 3 * hop - 1, 5000, 9217):
            x = torch.randn(n, generator=gen, dtype=torch.float64)
            got, want = R.magnitudes(x, n_fft, hop, pad_mode), _torch_mag(x, n_fft, hop, pad_mode)
            assert got.shape == want.shape == (n_fft // 2 + 1, 1 + n // hop)
            assert float((got - want).abs().max()) < 1e-11 * float(want.abs().max())
    if pad_mode == "constant":                              # clips shorter than half a window: constant padding only
        for n in (1, 2, 300):
            x = torch.randn(n, generator=gen, dtype=torch.float64)
            for n_fft, hop in ((R.MSE_N_FFT, R.MSE_HOP), (R.BAND_N_FFT, R.BAND_HOP)):
                assert float((R.magnitudes(x, n_fft, hop, pad_mode) - _torch_mag(x, n_fft, hop, pad_mode)).abs().max()) < 1e-11


@pytest.mark.parametrize("pad_mode", ["constant", "reflect"])
def test_restated_metrics_equal_the_reference_formulas(pad_mode):
    """evaluation_reconstruction.py:105-118 / :193-204 and evaluation_style_transfer.py:111-119 written with numpy on torch.stft"""
    gen = torch.Generator().manual_seed(23)
    a, g = torch.randn(7001, generator=gen), torch.randn(5200, generator=gen)
    L = min(len(a), len(g))
    so, sg = (_torch_mag(x[:L], 1024, 256, pad_mode).numpy() for x in (a, g))
    assert abs(float(R.mse_spectrogram(a, g, pad_mode)) / float(np.mean((so - sg) ** 2)) - 1) < 1e-12
    e1, e2 = (np.sum(_torch_mag(x, 2048, 512, pad_mode).numpy(), axis=1) for x in (a, g))
    assert abs(float(R.instrumentation_similarity(a, g, pad_mode)) - float(np.corrcoef(e1, e2)[0, 1])) < 1e-12
    assert float(R.pearson(torch.ones(1025, dtype=torch.float64), torch.from_numpy(e2))) == 0.0       # nan -> 0.0


def test_entries_are_declared_and_exported():
    for name in ("ast_spec_mse_len", "ast_spec_mse_ws_floats", "ast_band_energy_len", "ast_band_energy_ws_floats",
                 "ast_band_energy_run_frames", "ast_pearson_rows"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    assert ast_amd.mse_spectrogram is M.mse_spectrogram and ast_amd.band_energy is M.band_energy
    assert ast_amd.instrumentation_similarity is M.instrumentation_similarity


def test_workspace_counts():
    lib = _lib.lib()
    run = lib.ast_band_energy_run_frames()
    assert run >= 1
    assert lib.ast_spec_mse_ws_floats(4, 40000, 39000) == 4 * -(-(1 + 39000 // 256) // 2)
    assert lib.ast_band_energy_ws_floats(4, 40000) == 4 * -(-(1 + 40000 // 512) // run) * 1025
    assert lib.ast_spec_mse_ws_floats(0, 5, 5) == 0 and lib.ast_band_energy_ws_floats(3, 0) == 0


def _refused(rc, entry, needle):
    err = _lib.lib().ast_last_error()
    assert rc != 0 and entry in err and needle in err, (rc, err)


def test_entries_refuse_bad_arguments():
    lib = _lib.lib()

    def mse(**kw):
        a = dict(o=FAKE, no=40000, g=FAKE, ng=39000, B=4, lo=FAKE, lg=FAKE, pad=0, ws=FAKE, wsn=4 * 77, out=FAKE)
        a.update(kw)
        return lib.ast_spec_mse_len(a["o"], a["no"], a["g"], a["ng"], a["B"], a["lo"], a["lg"], a["pad"], a["ws"], a["wsn"], a["out"], None)

    for kw, needle in ((dict(o=None), b"null"), (dict(g=None), b"null"), (dict(out=None), b"null"), (dict(B=0), b"bad shape"),
                       (dict(B=65536), b"bad shape"), (dict(no=0), b"bad shape"), (dict(ng=-3), b"bad shape"), (dict(pad=2), b"pad_mode"),
                       (dict(pad=-1), b"pad_mode"), (dict(pad=1, ng=512), b"reflect"), (dict(pad=1, no=512), b"reflect"),
                       (dict(no=2 ** 31 - 2048), b"too long"), (dict(ws=None), b"workspace"), (dict(wsn=4 * 77 - 1), b"workspace")):
        _refused(mse(**kw), b"ast_spec_mse_len", needle)

    run = lib.ast_band_energy_run_frames()
    need = 4 * -(-79 // run) * 1025

    def band(**kw):
        a = dict(w=FAKE, B=4, n=40000, ns=FAKE, pad=0, ws=FAKE, wsn=need, e=FAKE)
        a.update(kw)
        return lib.ast_band_energy_len(a["w"], a["B"], a["n"], a["ns"], a["pad"], a["ws"], a["wsn"], a["e"], None)

    for kw, needle in ((dict(w=None), b"null"), (dict(e=None), b"null"), (dict(B=0), b"bad shape"), (dict(B=65536), b"bad shape"),
                       (dict(n=0), b"bad shape"), (dict(pad=7), b"pad_mode"), (dict(pad=1, n=1024), b"reflect"),
                       (dict(n=2 ** 31 - 4096), b"too long"), (dict(ws=None), b"workspace"), (dict(wsn=need - 1), b"workspace")):
        _refused(band(**kw), b"ast_band_energy_len", needle)

    for args, needle in (((None, FAKE, 4, 1025, FAKE), b"null"), ((FAKE, None, 4, 1025, FAKE), b"null"), ((FAKE, FAKE, 4, 1025, None), b"null"),
                         ((FAKE, FAKE, 0, 1025, FAKE), b"bad shape"), ((FAKE, FAKE, 4, 1, FAKE), b"bad shape"),
                         ((FAKE, FAKE, 65536, 65536, FAKE), b"bad shape")):
        _refused(lib.ast_pearson_rows(*args, None), b"ast_pearson_rows", needle)


def test_valid_calls_pass_the_checks_up_to_the_launch():
    """NULL lengths are valid (full rows).  Without a device the failure is the runtime's, with one the calls run on zeros."""
    lib = _lib.lib()
    if torch.cuda.is_available():
        w, ws, out = torch.zeros(2, 3000, device="cuda"), torch.zeros(4096 * 4, device="cuda"), torch.zeros(2 * 1025, device="cuda")
        for pad in (0, 1):
            assert lib.ast_spec_mse_len(w.data_ptr(), 3000, w.data_ptr(), 3000, 2, None, None, pad, ws.data_ptr(), ws.numel(), out.data_ptr(), None) == 0
            assert lib.ast_band_energy_len(w.data_ptr(), 2, 3000, None, pad, ws.data_ptr(), ws.numel(), out.data_ptr(), None) == 0
        torch.cuda.synchronize()
        return
    for rc in (lib.ast_spec_mse_len(FAKE, 3000, FAKE, 3000, 2, None, None, 1, FAKE, 10 ** 6, FAKE, None),
               lib.ast_band_energy_len(FAKE, 2, 3000, None, 1, FAKE, 10 ** 6, FAKE, None)):
        err = lib.ast_last_error()
        assert rc != 0
        for word in (b"bad", b"null", b"too long", b"reflect", b"workspace", b"pad_mode"):
            assert word not in err, err


def test_python_wrappers_refuse_bad_inputs():
    ok = torch.zeros(2, 3000)
    for fn, args in ((M.mse_spectrogram, (ok.double(), ok)), (M.mse_spectrogram, (ok, ok[0])), (M.mse_spectrogram, (ok, torch.zeros(3, 3000))),
                     (M.mse_spectrogram, (ok, np.zeros((2, 3000), dtype=np.float32))), (M.band_energy, (ok.half(),)),
                     (M.band_energy, (torch.zeros(2, 2, 3000),)), (M.band_energy, (torch.zeros(2, 0),)),
                     (M.instrumentation_similarity, (ok, torch.zeros(1, 3000))), (M.instrumentation_similarity, (ok.long(), ok))):
        with pytest.raises(ValueError):
            fn(*args)
    with pytest.raises(ValueError, match="pad_mode"):
        M.band_energy(ok, pad_mode="edge")
    with pytest.raises(ValueError, match="513"):
        M.mse_spectrogram(ok, torch.zeros(2, 512), pad_mode="reflect")
    with pytest.raises(ValueError, match="1025"):
        M.band_energy(torch.zeros(2, 1024), pad_mode="reflect")
    with pytest.raises(ValueError, match="1025"):
        M.instrumentation_similarity(ok, torch.zeros(2, 1024), pad_mode="reflect")
    for bad in (torch.zeros(2), torch.zeros(2, dtype=torch.int64), torch.zeros(3, dtype=torch.int32), [3000, 3000]):
        with pytest.raises(ValueError, match="n_samples"):
            M.band_energy(ok, bad)
    with pytest.raises(ValueError, match="n_generated"):
        M.mse_spectrogram(ok, ok, None, torch.zeros(2, dtype=torch.int32))              # a host tensor
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="device tensors"):                        # no CPU path
            M.band_energy(ok)


def test_transfer_and_score_argument_errors():
    from ast_amd.infer import StyleTransferSession
    sess = StyleTransferSession(torch.nn.Identity(), torch.nn.Identity(), use_graph=False)
    cls = torch.zeros(2, 256)
    with pytest.raises(ValueError, match="one or two channels"):                         # transfer's own checks come first
        sess.transfer_and_score(torch.zeros(2, 3, 90000), cls, sample_rate=48000)
    with pytest.raises(ValueError, match="cuda"):
        sess.transfer_and_score(torch.zeros(2, 90000), cls)


def test_seeds_show_an_ignored_length_or_pad_mode():
    """On the fixture of the GPU tests, by the float64 restatement alone: taking a shortened row as full moves every metric of
    that row by more than 100 x the tolerance, and so does the other pad mode on every row -- a kernel that ignores a count or
    the pad flag cannot pass the comparison.  The tolerance (10 x the float32 floor) is itself below 1e-5."""
    for pad_mode in ("constant", "reflect"):
        ref, full, bound = R.references(pad_mode), R.references(pad_mode, use_lengths=False), R.bounds(pad_mode)
        floor = R.f32_floor(pad_mode)
        print(f"{pad_mode}: float32 floor {floor}, bound {bound}, well-conditioned rows {R.conditioned_rows(pad_mode)}")
        assert all(0 < v < 1e-5 for v in bound.values()), bound
        for b in range(R.B):
            short = R.COUNTS[pad_mode][b] < R.N_MAX
            if short or R.N_GENERATED[b] < R.N_MAX:
                assert abs(float(full["mse"][b] / ref["mse"][b]) - 1) > 100 * bound["mse"], (pad_mode, b)
                if b in R.conditioned_rows(pad_mode):
                    assert abs(float(full["sim"][b] - ref["sim"][b])) > 100 * bound["sim"], (pad_mode, b)
            if short:
                assert R._rel(full["energy"][b], ref["energy"][b]) > 100 * bound["energy"], (pad_mode, b)
    # the pad mode, on the counts both modes accept
    a, g = R.fixture_waves()
    na = R.COUNTS["reflect"]
    bound = {k: max(R.bounds("constant")[k], R.bounds("reflect")[k]) for k in ("mse", "energy", "sim")}
    for b in range(R.B):
        L = min(na[b], max(R.N_GENERATED[b], 513))
        mc, mr = (float(R.mse_spectrogram(a[b, :L], g[b, :L], pm)) for pm in ("constant", "reflect"))
        ec, er = (R.band_energy(a[b, :na[b]], pm) for pm in ("constant", "reflect"))
        sc, sr = (float(R.instrumentation_similarity(a[b, :na[b]], g[b, :max(R.N_GENERATED[b], 1025)], pm)) for pm in ("constant", "reflect"))
        print(f"row {b}: constant against reflect: mse {abs(mc / mr - 1):.3g}, energy {R._rel(ec, er):.3g}, similarity {abs(sc - sr):.3g}")
        assert abs(mc / mr - 1) > 100 * bound["mse"] and R._rel(ec, er) > 100 * bound["energy"] and abs(sc - sr) > 100 * bound["sim"], b
    # the three cases of the band-energy kernel's runs are there (tests/test_gpu_metrics.py asserts the same)
    run = _lib.lib().ast_band_energy_run_frames()
    frames = sorted({R.n_frames(n, R.BAND_HOP) for counts in R.COUNTS.values() for n in counts})
    assert any(T < run for T in frames) and any(T >= run and T % run == 0 for T in frames) and any(T > run and T % run for T in frames), (run, frames)
