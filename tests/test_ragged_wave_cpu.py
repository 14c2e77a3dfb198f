"""Ragged waveforms without a GPU: the length arithmetic of the front end (csrc/ast_lengths.h through its host twin
ast_frontend_lengths_host) against section_starts, the host argument checks of the new entry points (every bad call is refused
before any launch), pad_waveforms, StyleEncoder's training-mode refusal, and the clips and oracle references that
tests/test_gpu_ragged_wave.py compares the kernels against -- with the check that an ignored length would show on them.

test_masked_style_transformer_reduces_to_the_oracle checks a float64 restatement and is the one test in this file that does
not depend on the feature."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from ast_amd import _lib
from ast_amd import utilityFunctions as U
from oracle import ast_oracle as O
from oracle import cqt_oracle as CO
from oracle import frontend_oracle as FO
from oracle import layout as OL

FAKE = 0x10000                                            # an aligned non-null pointer; nothing dereferences it
WIN, STEP, HOP = 287, 191, 256
NS_MIN = 36608                                            # max(513, 256 * ((287 + 1) // 2 - 1))
# (samples, kind): full width with 2 sections; 1 section and a dropped tail (frames 287..300); the minimum plus 100, one partly
# filled section, no multiple of 256; an odd count, so that ceil matters in every halving
CLIPS = ((85760, "piano"), (76800, "violin"), (NS_MIN + 100, "piano"), (60001, "violin"))
NS = [c[0] for c in CLIPS]
N_MAX = max(NS)
STFT_BOUND = lambda scale: 2e-5 * scale + 2e-5            # noqa: E731  tests/test_gpu_ops.py::test_stft_frontend
CQT_BOUND = lambda peak: 2e-5 * peak                      # noqa: E731  tests/test_gpu_ops.py::test_cqt_matches_oracle


def host_lengths(ns, nsamp=N_MAX):
    """(clamped ns, T, n_sec, n_frames) in plain Python: the statement of the rules, not the header"""
    ns = min(max(ns, NS_MIN), nsamp)
    T = 1 + ns // HOP
    n = len(U.section_starts(T))
    return ns, T, n, min(T, STEP * (n - 1) + WIN)


@functools.lru_cache(maxsize=None)
def clip_waves():
    """the four clips, cut from seeded 4 s syntheses"""
    return [FO.synth_waveform(i, kind, 4.0)[:ns].copy() for i, (ns, kind) in enumerate(CLIPS)]


def _sections(w):
    """oracle front end without statistics: (S, 2, 287, 513) STFT sections and (S, 2, 287, 84) CQT sections of one waveform"""
    return FO.overlap_windows(FO.stft(w)), FO.overlap_windows(CO.get_cqt(w))


@functools.lru_cache(maxsize=None)
def solo_oracle():
    """every clip alone through the oracle front end"""
    return [_sections(w) for w in clip_waves()]


def _zero_extended(a, S):
    out = np.zeros((S,) + a.shape[1:], dtype=a.dtype)
    out[:a.shape[0]] = a
    return out


# ---- length arithmetic ---------------------------------------------------------------------------------------------------------
def test_the_three_clips_have_the_counts_the_tests_rely_on():
    assert host_lengths(85760) == (85760, 336, 2, 336)
    assert host_lengths(76800) == (76800, 301, 1, 287)            # frames 287..300 are a dropped tail
    assert host_lengths(NS_MIN + 100) == (NS_MIN + 100, 144, 1, 144)
    assert host_lengths(60001) == (60001, 235, 1, 235)
    assert U.section_starts(143) == [] and U.section_starts(144) == [0]


def test_length_function_against_section_starts():
    """The header's function (the one the kernels compile) for every T in 144 .. 1200, at the first and last sample count
    of that T, and its clamping to [NS_MIN, nsamp]."""
    nsamp = 256 * 1200
    for T in range(144, 1201):
        for ns in (256 * (T - 1), 256 * (T - 1) + 255):
            starts = U.section_starts(T)
            assert U.clip_lengths(ns, nsamp) == (ns, T, len(starts), min(T, STEP * (len(starts) - 1) + WIN)), (T, ns)
            assert U.clip_lengths(ns, nsamp) == host_lengths(ns, nsamp)
    for ns in (-7, 0, 5, NS_MIN - 1):
        assert U.clip_lengths(ns, N_MAX) == U.clip_lengths(NS_MIN, N_MAX) == (NS_MIN, 144, 1, 144)
    for ns in (N_MAX + 1, 10 ** 6, 2 ** 31 - 1):
        assert U.clip_lengths(ns, N_MAX) == U.clip_lengths(N_MAX, N_MAX) == (85760, 336, 2, 336)
    with pytest.raises(RuntimeError, match="ast_frontend_lengths_host"):
        U.clip_lengths(50000, NS_MIN - 1)                              # the padded row itself is too short
    # ceil-halving o times is ceil(ns / 2^o): what the masked decimation and the octave kernel assume
    for ns in (60001, NS_MIN + 100, 85760):
        m = ns
        for o in range(1, 7):
            m = (m + 1) // 2
            assert m == -(-ns // 2 ** o)


# ---- host argument checks --------------------------------------------------------------------------------------------------------
def _refused(lib, rc, name, needle, what):
    assert rc != 0, what
    err = lib.ast_last_error()
    assert name in err and needle in err, (what, err)


def test_frontend_lengths_and_stft_len_refuse_bad_arguments():
    lib, f = _lib.lib(), FAKE
    ok = dict(n=f, Bc=3, nsamp=N_MAX, win=WIN, step=STEP, a=f, b=f)
    for kw, needle in ((dict(n=None), b"n_samples"), (dict(a=None), b"null"), (dict(b=None), b"null"), (dict(Bc=0), b"bad shape"),
                       (dict(step=0), b"bad shape"), (dict(step=288), b"bad shape"), (dict(nsamp=NS_MIN - 1), b"needs")):
        a = dict(ok, **kw)
        rc = lib.ast_frontend_lengths(a["n"], a["Bc"], a["nsamp"], a["win"], a["step"], a["a"], a["b"], None)
        _refused(lib, rc, b"ast_frontend_lengths", needle, kw)
    ok = dict(wave=f, Bc=3, nsamp=N_MAX, mean=f, std=f, x=f, S=2, win=WIN, step=STEP, F=597, n=f)
    for kw, needle in ((dict(n=None), b"n_samples"), (dict(wave=None), b"bad args"), (dict(mean=None), b"bad args"),
                       (dict(x=None), b"bad args"), (dict(Bc=0), b"bad args"), (dict(S=0), b"bad args"), (dict(F=512), b"bad args"),
                       (dict(nsamp=512), b"bad args"), (dict(step=0), b"bad args"), (dict(nsamp=NS_MIN - 1), b"needs"),
                       (dict(nsamp=20000), b"needs")):
        a = dict(ok, **kw)
        rc = lib.ast_stft_sections_len(a["wave"], a["Bc"], a["nsamp"], a["mean"], a["std"], a["x"], a["S"], a["win"], a["step"],
                                       a["F"], a["n"], None)
        _refused(lib, rc, b"ast_stft_sections_len", needle, kw)


def _octave_args(no=7, nsamp=N_MAX, ns=None, ys=None):
    I = ctypes.c_int * no
    ns = [-(-nsamp // 2 ** o) for o in range(no)] if ns is None else ns
    ys = [FAKE] * no if ys is None else ys
    return ((ctypes.c_void_p * no)(*ys), I(*ns), I(*[256 >> o for o in range(no)]), I(*[72 - 12 * o for o in range(no)]),
            I(*[12] * no), I(*[0] * no))


def test_cqt_len_entries_refuse_bad_arguments():
    lib, f = _lib.lib(), FAKE
    ok = dict(x=f, B=3, n=N_MAX, h=f, klen=359, width=179, y=f, m=N_MAX // 2, gain=1.0, ns=f, nsamp=N_MAX, win=WIN, step=STEP, o=0)
    for kw, needle in ((dict(ns=None), b"n_samples"), (dict(x=None), b"null"), (dict(h=None), b"null"), (dict(y=None), b"null"),
                       (dict(B=0), b"bad shape"), (dict(klen=4097), b"bad shape"), (dict(m=0), b"bad shape"), (dict(o=-1), b"bad shape"),
                       (dict(o=1), b"halved"), (dict(n=N_MAX - 1), b"halved"), (dict(nsamp=NS_MIN - 1, n=NS_MIN - 1), b"needs"),
                       (dict(step=0), b"sectioning")):
        a = dict(ok, **kw)
        rc = lib.ast_decimate2_len(a["x"], a["B"], a["n"], a["h"], a["klen"], a["width"], a["y"], a["m"], a["gain"], a["ns"], a["nsamp"],
                                   a["win"], a["step"], a["o"], None)
        _refused(lib, rc, b"ast_decimate2_len", needle, kw)

    def octaves(arrs=None, n_oct=7, B=3, w=f, nfft=256, out=f, T=336, ld=597, bin_off=513, n=f, nsamp=N_MAX, win=WIN, step=STEP):
        arrs = _octave_args() if arrs is None else arrs
        return lib.ast_cqt_octaves_len(*arrs, n_oct, B, w, f, f, nfft, out, T, ld, bin_off, n, nsamp, win, step, None)

    for kw, needle in ((dict(n=None), b"n_samples"), (dict(w=None), b"null"), (dict(out=None), b"null"), (dict(n_oct=13), b"bad shape"),
                       (dict(B=0), b"bad shape"), (dict(nfft=255), b"bad shape"), (dict(T=0), b"bad shape"), (dict(ld=596), b"bad octave"),
                       (dict(arrs=_octave_args(ns=[N_MAX] * 7)), b"halved"), (dict(arrs=_octave_args(ys=[FAKE] * 6 + [None])), b"bad octave"),
                       (dict(nsamp=NS_MIN - 1), b"needs"), (dict(win=0), b"sectioning")):
        _refused(lib, octaves(**kw), b"ast_cqt_octaves_len", needle, kw)

    ok = dict(c=f, Bc=3, T=336, nb=84, mean=f, std=f, x=f, S=2, win=WIN, step=STEP, F=597, bin0=513, n=f, nsamp=N_MAX)
    for kw, needle in ((dict(n=None), b"n_samples"), (dict(c=None), b"null"), (dict(x=None), b"null"), (dict(Bc=0), b"bad shape"),
                       (dict(bin0=514), b"bad shape"), (dict(S=0), b"bad shape"), (dict(T=335), b"1 + nsamp"), (dict(nsamp=NS_MIN - 1, T=143), b"needs")):
        a = dict(ok, **kw)
        rc = lib.ast_cqt_sections_len(a["c"], a["Bc"], a["T"], a["nb"], a["mean"], a["std"], a["x"], a["S"], a["win"], a["step"], a["F"],
                                      a["bin0"], a["n"], a["nsamp"], None)
        _refused(lib, rc, b"ast_cqt_sections_len", needle, kw)


def test_valid_calls_pass_the_checks_up_to_the_launch():
    """A valid call is refused by none of the checks: without a device the launch itself fails with the runtime's message, with
    one the calls run on zeroed buffers that are large enough (zero lengths are clamped to NS_MIN)."""
    lib = _lib.lib()
    gpu = torch.cuda.is_available()
    if gpu:
        bufs = [torch.zeros(3 * 2 * 2 * WIN * 597, device="cuda") for _ in range(3)]
        lens = torch.zeros(8, dtype=torch.int32, device="cuda")
        a, b, c = (t.data_ptr() for t in bufs)
        n = lens.data_ptr()
        ys = [torch.zeros(3 * -(-N_MAX // 2 ** o), device="cuda") for o in range(7)]
        arrs = _octave_args(ys=[t.data_ptr() for t in ys])
    else:
        a = b = c = n = FAKE
        arrs = _octave_args()
    calls = [lambda: lib.ast_frontend_lengths(n, 3, N_MAX, WIN, STEP, a, b, None),
             lambda: lib.ast_stft_sections_len(a, 3, N_MAX, b, b, c, 2, WIN, STEP, 597, n, None),
             lambda: lib.ast_decimate2_len(a, 3, N_MAX, b, 359, 179, c, N_MAX // 2, 1.0, n, N_MAX, WIN, STEP, 0, None),
             lambda: lib.ast_cqt_octaves_len(*arrs, 7, 3, a, a, a, 256, c, 336, 597, 513, n, N_MAX, WIN, STEP, None),
             lambda: lib.ast_cqt_sections_len(a, 3, 336, 84, b, b, c, 2, WIN, STEP, 597, 513, n, N_MAX, None)]
    for i, call in enumerate(calls):
        rc = call()
        if gpu:
            assert rc == 0, (i, lib.ast_last_error())
            continue
        assert rc != 0, i
        err = lib.ast_last_error()
        for word in (b"bad", b"needs", b"NULL", b"null", b"halved", b"1 + nsamp"):
            assert word not in err, (i, err)
    if gpu:
        torch.cuda.synchronize()


# ---- Python surface ----------------------------------------------------------------------------------------------------------------
def test_pad_waveforms():
    gen = torch.Generator().manual_seed(4)
    clips = [torch.randn(5, generator=gen), torch.randn(1, 9, generator=gen), torch.randn(7, generator=gen)]
    waves, n = U.pad_waveforms(clips)
    assert waves.shape == (3, 9) and waves.dtype == torch.float32 and n.dtype == torch.int32 and n.tolist() == [5, 9, 7]
    for b, c in enumerate(clips):
        assert torch.equal(waves[b, :n[b]], c.reshape(-1)) and float(waves[b, n[b]:].abs().sum()) == 0.0
    for bad in ([], [torch.zeros(2, 9)], [torch.zeros(3, 1, 1)], [torch.zeros(5), torch.zeros(5, dtype=torch.float64)],
                [torch.zeros(0)], [torch.zeros(5), np.zeros(5, dtype=np.float32)]):
        with pytest.raises(ValueError):
            U.pad_waveforms(bad)


def test_lengths_in_training_mode_is_a_value_error():
    import ast_amd
    n = torch.tensor([1, 1], dtype=torch.int32)
    for use_cls in (True, False):
        enc = ast_amd.StyleEncoder(use_cls=use_cls).train()
        with pytest.raises(ValueError, match="inference"):
            enc(torch.zeros(2, 1, 2, 287, 597), None, n)
        with pytest.raises(ValueError, match="int32"):
            enc.eval()(torch.zeros(2, 1, 2, 287, 597), lengths=torch.tensor([1, 1]))


# ---- an ignored length cannot pass the device tests ----------------------------------------------------------------------------------
def test_zero_padded_waveforms_miss_the_device_bounds():
    """The device tests bound row b of the padded batch by the oracle on the clip alone (STFT 2e-5 of scale + 2e-5, CQT 2e-5 of
    the peak) and assert that the unchanged entries miss.  Here the oracle says that these seeded clips make it so: the
    zero-padded waveform through the oracle front end differs from the clip alone (its sections, 0 behind them) by far more than
    those bounds for every clip shorter than the row -- the reflection at the clip's end, the FIR's ringing past a halving's
    truncation, and the dropped tail that a padded row turns into a section."""
    solo = solo_oracle()
    S = len(U.section_starts(1 + N_MAX // HOP))
    for b, w in enumerate(clip_waves()):
        padded = np.zeros(N_MAX, dtype=np.float32)
        padded[:NS[b]] = w
        st, cq = _sections(padded)
        _, _, n_sec, _ = host_lengths(NS[b])
        assert solo[b][0].shape[0] == n_sec and st.shape[0] == S
        gap_st = float(np.abs(st - _zero_extended(solo[b][0], S)).max())
        gap_cq = float(np.abs(cq - _zero_extended(solo[b][1], S)).max())
        # the clip's own last section alone already shows it, in the CQT bins (whose low octaves reach 8192 samples back from
        # the clip's end; the STFT's frames of a dropped-tail clip end before it, there the spurious section shows)
        last = n_sec - 1
        gap_last = float(np.abs(cq[last] - solo[b][1][last]).max())
        bound_st, bound_cq = STFT_BOUND(float(np.abs(solo[b][0]).max())), CQT_BOUND(float(np.abs(solo[b][1]).max()))
        print(f"clip {b} ns={NS[b]}: padded against solo STFT {gap_st:.3g} (bound {bound_st:.3g}), CQT {gap_cq:.3g} (bound {bound_cq:.3g}), "
              f"CQT of its last own section {gap_last:.3g}")
        if NS[b] == N_MAX:
            assert gap_st == 0.0 and gap_cq == 0.0
        else:
            assert gap_st > 10 * bound_st and gap_cq > 10 * bound_cq and gap_last > 10 * bound_cq, b


# ---- float64 restatement of StyleEncoder's transformer with a length mask ----------------------------------------------------------------
def style_transformer_f64(sd, feat, lengths, use_cls=True, nhead=4, nlayers=4):
    """style_encoder.py:199-241 after the CNN in float64, clip b seeing its first lengths[b] section tokens only: (B, S, d)
    CNN features -> (B, d) style embeddings (the CLS row, or the mean over the clip's own rows)."""
    d64 = lambda k: sd[k].detach().double()                   # noqa: E731
    B, S, d = feat.shape
    seq = feat.double()
    if use_cls:
        seq = torch.cat([d64("cls_token").expand(B, -1, -1), seq], dim=1)
    L = seq.shape[1]
    valid = torch.arange(L)[None, :] < (torch.as_tensor(lengths)[:, None] + (1 if use_cls else 0))          # a prefix: CLS is token 0
    ln = lambda x, p: torch.nn.functional.layer_norm(x, (d,), d64(p + "weight"), d64(p + "bias"), 1e-5)       # noqa: E731
    seq = ln(seq + O.positional_encoding(L, d).double(), "norm.")
    dh = d // nhead
    for i in range(nlayers):
        p = f"transformer.layers.{i}."
        w, bias = d64(p + "self_attn.in_proj_weight"), d64(p + "self_attn.in_proj_bias")
        q, k, v = ((seq @ w[j * d:(j + 1) * d].t() + bias[j * d:(j + 1) * d]).view(B, L, nhead, dh).transpose(1, 2) for j in range(3))
        s = (q @ k.transpose(-1, -2)) / math.sqrt(dh)
        s = s.masked_fill(~valid[:, None, None, :], float("-inf"))
        a = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, L, d)
        seq = ln(seq + a @ d64(p + "self_attn.out_proj.weight").t() + d64(p + "self_attn.out_proj.bias"), p + "norm1.")
        h = torch.relu(seq @ d64(p + "linear1.weight").t() + d64(p + "linear1.bias"))
        seq = ln(seq + h @ d64(p + "linear2.weight").t() + d64(p + "linear2.bias"), p + "norm2.")
    if use_cls:
        return seq[:, 0]
    return (seq * valid[:, :, None]).sum(1) / valid.sum(1, keepdim=True)


def test_masked_style_transformer_reduces_to_the_oracle():
    """At full lengths the masked restatement is the oracle's unmasked stack; with short lengths a clip equals the same clip
    cut to its length, whatever the padded rows hold."""
    sd = OL.seeded_model_state("style", requires_grad=False)
    gen = torch.Generator().manual_seed(11)
    feat = torch.randn(3, 3, 256, generator=gen)
    cfg = O.Cfg(training=False)
    with torch.no_grad():
        seq = torch.cat([sd["cls_token"].expand(3, -1, -1), feat], dim=1)
        ref_cls = O._encoder_stack(sd, O.layernorm(sd, "norm.", seq + O.positional_encoding(4, 256)), 4, 4, cfg)[:, 0]
        ref_mean = O._encoder_stack(sd, O.layernorm(sd, "norm.", feat + O.positional_encoding(3, 256)), 4, 4, cfg).mean(1)
        for use_cls, ref in ((True, ref_cls), (False, ref_mean)):
            full = style_transformer_f64(sd, feat, [3, 3, 3], use_cls)
            assert float((full - ref.double()).abs().max() / ref.abs().max()) < 1e-5, use_cls
            noisy = feat.clone()
            noisy[1, 1:], noisy[2, 2:] = 1e3, -1e3
            short = style_transformer_f64(sd, noisy, [3, 1, 2], use_cls)
            for b, n in enumerate((3, 1, 2)):
                alone = style_transformer_f64(sd, feat[b:b + 1, :n], [n], use_cls)
                assert float((short[b:b + 1] - alone).abs().max()) < 1e-12, (use_cls, b)
