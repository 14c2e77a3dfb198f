"""Ragged inference batches without a GPU: the host argument checks of the three length-aware entry points (every bad call is
refused before any launch), the bookkeeping of pad_sections / the per-clip default frame count, the float64 numpy
restatement of the three masked operations that tests/test_gpu_ragged.py compares the kernels against, and the inputs and
oracle references of its model tests, with the check that a missing mask would show on them.

test_restatements_reduce_to_the_unmasked_operations checks the restatements themselves (against torch, the front-end oracle
and hand-picked sums), so it alone in this file does not depend on the feature."""
import functools

import numpy as np
import pytest
import torch

from ast_amd import _lib
from ast_amd import utilityFunctions as U
from oracle import ast_oracle as O
from oracle import layout as OL
from oracle import seeded_params as sp

FAKE = 0x10000                                            # a 16-byte aligned non-null pointer; nothing dereferences it
NFFT, HOP, WIND, STEP = 1024, 256, 287, 191


# ---- float64 restatements ----------------------------------------------------------------------------------------------------
def masked_attention_f64(q, k, v, B, H, Lq, Lk, dh, causal, key_len, key_period):
    """softmax(Q K^T / sqrt(dh)) V over the keys j with (j % key_period) < clamp(key_len[b], 1, key_period); masked keys
    take no part at all (their rows are not read, so NaN there is harmless) and get probability 0.
    q: (B*Lq, H*dh), k, v: (B*Lk, H*dh) -> o (B*Lq, H*dh), probs (B, H, Lq, Lk)."""
    q, k, v = (np.asarray(t, dtype=np.float64) for t in (q, k, v))
    Q = q.reshape(B, Lq, H, dh).transpose(0, 2, 1, 3)
    K = k.reshape(B, Lk, H, dh).transpose(0, 2, 1, 3)
    V = v.reshape(B, Lk, H, dh).transpose(0, 2, 1, 3)
    o = np.zeros((B, H, Lq, dh))
    probs = np.zeros((B, H, Lq, Lk))
    for b in range(B):
        kl = min(max(int(key_len[b]), 1), key_period)
        keys = np.array([j for j in range(Lk) if j % key_period < kl])
        s = Q[b] @ K[b][:, keys].transpose(0, 2, 1) / np.sqrt(dh)                 # (H, Lq, nkeys)
        if causal:
            s = np.where(keys[None, None, :] > np.arange(Lq)[None, :, None], -np.inf, s)
        p = np.exp(s - s.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        probs[b][:, :, keys] = p
        o[b] = p @ V[b][:, keys]
    return o.transpose(0, 2, 1, 3).reshape(B * Lq, H * dh), probs


def overlap_avg_f64(sections, n_sec, n_frames, hop, out_T):
    """(B, S, 2, wind, F) -> (B, 2, out_T, F): clip b averages its sections k < n_sec[b]; frames t >= n_frames[b] are 0."""
    sec = np.asarray(sections, dtype=np.float64)
    B, S, _, wind, F = sec.shape
    out = np.zeros((B, 2, out_T, F))
    for b in range(B):
        ns, nf = min(max(int(n_sec[b]), 1), S), min(max(int(n_frames[b]), 1), out_T)
        acc, cnt = np.zeros((2, out_T + wind, F)), np.zeros(out_T + wind)
        for k in range(ns):
            if k * hop >= out_T:
                break
            acc[:, k * hop:k * hop + wind] += sec[b, k]
            cnt[k * hop:k * hop + wind] += 1
        out[b, :, :nf] = (acc / np.maximum(cnt, 1)[None, :, None])[:, :nf]
    return out


def istft_f64(spec, n_frames):
    """(B, 2, T, 513) -> (B, 256 (T - 1)): clip b inverted as a clip of Tb = clamp(n_frames[b], 2, T) frames (torch.istft
    defaults: periodic Hann, window^2 envelope, centre trimmed); samples from 256 (Tb - 1) on are 0."""
    spec = np.asarray(spec, dtype=np.float64)
    B, _, T, _ = spec.shape
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(NFFT) / NFFT)
    wave = np.zeros((B, HOP * (T - 1)))
    for b in range(B):
        Tb = min(max(int(n_frames[b]), 2), T)
        frames = np.fft.irfft(spec[b, 0, :Tb] + 1j * spec[b, 1, :Tb], n=NFFT, axis=1) * win[None, :]
        L = NFFT + HOP * (Tb - 1)
        y, env = np.zeros(L), np.zeros(L)
        for t in range(Tb):
            y[t * HOP:t * HOP + NFFT] += frames[t]
            env[t * HOP:t * HOP + NFFT] += win ** 2
        y, env = y[NFFT // 2:L - NFFT // 2], env[NFFT // 2:L - NFFT // 2]
        wave[b, :HOP * (Tb - 1)] = y / np.where(env > 1e-11, env, 1.0)
    return wave


def test_restatements_reduce_to_the_unmasked_operations():
    """With full lengths the three restatements are the plain operations (torch softmax attention, the frontend oracle's
    istft, a direct overlap-average); with short lengths a clip equals the same clip cut to its length."""
    from oracle import frontend_oracle as FO
    rng = np.random.default_rng(5)
    B, H, Lq, Lk, dh = 2, 2, 3, 6, 8
    q, k, v = rng.standard_normal((B * Lq, H * dh)), rng.standard_normal((B * Lk, H * dh)), rng.standard_normal((B * Lk, H * dh))
    o, p = masked_attention_f64(q, k, v, B, H, Lq, Lk, dh, False, [3, 3], 3)
    t = lambda a, L: torch.from_numpy(a).view(B, L, H, dh).transpose(1, 2)
    pr = torch.softmax(t(q, Lq) @ t(k, Lk).transpose(-1, -2) / np.sqrt(dh), -1)
    assert np.allclose(p, pr.numpy(), atol=1e-14)
    assert np.allclose(o, (pr @ t(v, Lk)).transpose(1, 2).reshape(B * Lq, H * dh).numpy(), atol=1e-13)
    # period 3 of 6 keys with key_len [2, 1]: batch 0 keeps keys {0, 1, 3, 4}, batch 1 keeps {0, 3}; NaN elsewhere is never read
    kn, vn = k.copy().reshape(B, Lk, -1), v.copy().reshape(B, Lk, -1)
    kn[0, [2, 5]] = vn[0, [2, 5]] = kn[1, [1, 2, 4, 5]] = vn[1, [1, 2, 4, 5]] = np.nan
    o2, p2 = masked_attention_f64(q, kn.reshape(B * Lk, -1), vn.reshape(B * Lk, -1), B, H, Lq, Lk, dh, False, [2, 1], 3)
    assert np.isfinite(o2).all() and np.isfinite(p2).all()
    assert (p2[0][:, :, [2, 5]] == 0).all() and (p2[1][:, :, [1, 2, 4, 5]] == 0).all() and np.allclose(p2.sum(-1), 1.0)
    o3, _ = masked_attention_f64(q, k, v, B, H, Lq, Lk, dh, False, [0, 10], 3)         # clamped to [1, 3]
    o4, _ = masked_attention_f64(q, k, v, B, H, Lq, Lk, dh, False, [1, 3], 3)
    assert np.array_equal(o3, o4)

    spec = rng.standard_normal((2, 2, 9, 513))
    w = istft_f64(spec, [9, 5])
    assert np.allclose(w[0], FO.istft(spec[0].astype(np.float32)), atol=1e-5)
    assert np.allclose(w[1, :HOP * 4], FO.istft(spec[1, :, :5].astype(np.float32)), atol=1e-5) and (w[1, HOP * 4:] == 0).all()

    sec = rng.standard_normal((2, 3, 2, 8, 4))                                          # wind 8, hop 5
    out = overlap_avg_f64(sec, [3, 2], [18, 11], 5, 18)
    assert np.allclose(out[0, :, 5:8], 0.5 * (sec[0, 0, :, 5:8] + sec[0, 1, :, 0:3])) and np.allclose(out[0, :, 13:], sec[0, 2, :, 3:])
    assert np.allclose(out[1, :, 8:10], sec[1, 1, :, 3:5]) and np.allclose(out[1, :, 10:11], sec[1, 1, :, 5:6])
    assert (out[1, :, 11:] == 0).all()


# ---- host argument checks ------------------------------------------------------------------------------------------------------
def _attn_len(lib, Lq=3, Lk=6, period=3, key_len=FAKE, dh=64, H=4, q=FAKE, ld=None):
    ld = H * dh if ld is None else ld
    return lib.ast_attn_fwd_len(q, FAKE, FAKE, FAKE, FAKE, 2, H, Lq, Lk, dh, ld, ld, ld, 0, key_len, period, None)


def test_attn_fwd_len_refuses_bad_arguments():
    lib = _lib.lib()

    def refused(needle, **kw):
        assert _attn_len(lib, **kw) != 0, kw
        err = lib.ast_last_error()
        assert b"ast_attn_fwd_len" in err and needle in err, (kw, err)

    refused(b"key_period", period=0)
    refused(b"key_period", period=7)                           # > Lk
    refused(b"key_period", period=4)                           # Lk % key_period != 0
    refused(b"key_period", period=-3)
    refused(b"key_len", key_len=None)
    refused(b"key_len", key_len=None, Lq=17, Lk=34, period=17)
    # everything ast_attn_fwd checks, on both paths
    refused(b"bad args", q=None)
    refused(b"dh", dh=65)
    refused(b"1<=L", Lq=0)
    refused(b"1024", Lq=1, Lk=1026, period=513)
    refused(b"dh % 4", dh=30, Lq=17, Lk=34, period=17)
    refused(b"16-byte", q=FAKE + 4, Lq=1, Lk=34, period=17)
    refused(b"multiple of 4", ld=258, Lq=17, Lk=34, period=17)
    refused(b"key_period", Lq=17, Lk=34, period=16)


def test_overlap_avg_len_and_istft_len_refuse_bad_arguments():
    lib = _lib.lib()
    f = FAKE
    ok = dict(sec=f, out=f, Bc=2, S=3, wind=287, hop=191, F_in=513, F_out=513, out_T=669, n_sec=f, n_frames=f)

    def avg(**kw):
        a = dict(ok, **kw)
        return lib.ast_sections_overlap_avg_len(a["sec"], a["out"], a["Bc"], a["S"], a["wind"], a["hop"], a["F_in"], a["F_out"],
                                                a["out_T"], a["n_sec"], a["n_frames"], None)

    for kw, needle in ((dict(n_sec=None), b"n_sec"), (dict(n_frames=None), b"n_frames"), (dict(sec=None), b"bad args"),
                       (dict(out_T=670), b"bad args"), (dict(out_T=0), b"bad args"), (dict(S=0), b"bad args"),
                       (dict(F_out=514), b"bad args"), (dict(hop=288), b"bad args"), (dict(Bc=0), b"bad args")):
        assert avg(**kw) != 0, kw
        err = lib.ast_last_error()
        assert b"ast_sections_overlap_avg_len" in err and needle in err, (kw, err)

    for args, needle in (((f, 2, 9, f, f, None), b"n_frames"), ((None, 2, 9, f, f, f), b"bad args"), ((f, 2, 1, f, f, f), b"bad args"),
                         ((f, 0, 9, f, f, f), b"bad args"), ((f, 2, 9, None, f, f), b"bad args"), ((f, 2, 9, f, None, f), b"bad args")):
        assert lib.ast_istft_len(*args, None) != 0, args
        err = lib.ast_last_error()
        assert b"ast_istft_len" in err and needle in err, (args, err)


def test_valid_shapes_pass_the_checks_up_to_the_launch():
    """A valid call is refused by none of the argument checks.  Without a device the launch itself fails, and the message is
    the runtime's, not one of the checks' ("needs", "bad args", ...); fake pointers are enough, nothing dereferences them.
    With a device the same calls run on real (zeroed, large enough) buffers and succeed: zero lengths are clamped."""
    lib = _lib.lib()
    gpu = torch.cuda.is_available()
    bufs = [torch.zeros(2 << 20, device="cuda") for _ in range(5)] if gpu else None
    lens = torch.zeros(8, dtype=torch.int32, device="cuda") if gpu else None
    q, k, v, o, p = (b.data_ptr() for b in bufs) if gpu else (FAKE,) * 5
    n = lens.data_ptr() if gpu else FAKE

    def attn(Lq, Lk, period, dh=64, H=4):
        return lib.ast_attn_fwd_len(q, k, v, o, p, 2, H, Lq, Lk, dh, H * dh, H * dh, H * dh, 0, n, period, None)

    calls = [lambda: attn(3, 6, 3), lambda: attn(8, 16, 8), lambda: attn(1, 34, 17), lambda: attn(17, 17, 17, dh=32),
             lambda: lib.ast_sections_overlap_avg_len(q, o, 2, 3, 287, 191, 513, 513, 669, n, n, None),
             lambda: lib.ast_istft_len(q, 2, 669, k, o, n, None)]
    for i, call in enumerate(calls):
        rc = call()
        if gpu:
            assert rc == 0, (i, lib.ast_last_error())
            continue
        assert rc != 0, i                                       # no device here: the launch fails
        err = lib.ast_last_error()
        for word in (b"bad args", b"needs", b"NULL", b"at most", b"16-byte"):
            assert word not in err, (i, err)
    if gpu:
        torch.cuda.synchronize()


# ---- bookkeeping -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seconds", [2, 3, 4, 5, 6, 7, 8, 9, 10])
def test_default_frames_match_section_starts(seconds):
    """A clip of `seconds` at 22 050 Hz has T = 1 + n // 256 frames and sections at section_starts(T); the per-clip default frame
    count the session forms on the device, 191 (n_b - 1) + 287, is the end of its last section: what its sections cover."""
    T = 1 + (seconds * 22050) // 256
    starts = U.section_starts(T)
    n = len(starts)
    assert starts == [STEP * k for k in range(n)]
    frames = int(U.default_frames(torch.tensor([n], dtype=torch.int32))[0])
    assert frames == starts[-1] + WIND == STEP * (n - 1) + WIND
    assert frames - T < WIND * 0.5 + 1e-9 or frames <= T          # a padded last section is padded by less than half a window
    assert T - frames < STEP                                        # and a dropped tail is shorter than one step


def test_pad_sections():
    gen = torch.Generator().manual_seed(3)
    clips = [torch.randn(n, 2, WIND, 5, generator=gen) for n in (3, 1, 2)]
    sec, n = U.pad_sections(clips)
    assert sec.shape == (3, 3, 2, WIND, 5) and n.dtype == torch.int32 and n.tolist() == [3, 1, 2]
    for b, c in enumerate(clips):
        assert torch.equal(sec[b, :c.shape[0]], c) and float(sec[b, c.shape[0]:].abs().max() if c.shape[0] < 3 else 0.0) == 0.0
    assert U.default_frames(n).tolist() == [669, 287, 478] and U.default_frames(n).dtype == torch.int32
    with pytest.raises(ValueError):
        U.pad_sections([])
    with pytest.raises(ValueError):
        U.pad_sections([clips[0], torch.zeros(2, 2, WIND, 6)])


def test_lengths_in_training_mode_is_a_value_error():
    """Per-clip lengths are an inference feature: both modules refuse them in training mode before touching the device."""
    import ast_amd
    n = torch.tensor([1, 1], dtype=torch.int32)
    dec = ast_amd.Decoder().train()
    with pytest.raises(ValueError, match="inference"):
        dec(torch.zeros(2, 1, 256), torch.zeros(2, 256), y=torch.zeros(2, 1, 2, 287, 513), lengths=n)
    with pytest.raises(ValueError, match="inference"):
        dec.prepare_memory(torch.zeros(2, 1, 256), torch.zeros(2, 256), lengths=n)
    with pytest.raises(ValueError, match="inference"):
        ast_amd.ContentEncoder().train()(torch.zeros(2, 1, 2, 287, 597), n)
    with pytest.raises(ValueError, match="int32"):
        ast_amd.Decoder().eval()(torch.zeros(2, 1, 256), torch.zeros(2, 256), lengths=torch.tensor([1, 1]))


# ---- inputs and oracle references of the model tests (tests/test_gpu_ragged.py, short path) --------------------------------------------
N_SHORT = [3, 1, 2]


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def short_inputs():
    """Three clips of N_SHORT sections, class embeddings, and (3, 3, 256) token rows: the decoder's content embeddings and the
    input of the content encoder's transformer stack.  Rows s >= n_b of the token rows are seeded noise like the others: with
    lengths nothing may depend on them, without lengths they leak in."""
    clips = [sp.seeded_input(1, n, seed=7300 + b)[0] for b, n in enumerate(N_SHORT)]
    return clips, sp.seeded_normal((3, 256), 7310), sp.seeded_normal((3, 3, 256), 7320)


@functools.lru_cache(maxsize=None)
def short_content_oracle():
    """The CPU oracle's content embeddings of every clip alone."""
    clips, _, _ = short_inputs()
    sd = OL.seeded_model_state("content", requires_grad=False)
    with torch.no_grad():
        return [O.content_encoder_forward(sd, c[None], O.Cfg(training=False)) for c in clips]


@functools.lru_cache(maxsize=None)
def short_transformer_oracle():
    """The content encoder's transformer stack (content_encoder.py:24-26) on each clip's own token rows."""
    _, _, rows = short_inputs()
    sd = OL.seeded_model_state("content", requires_grad=False)
    with torch.no_grad():
        return [O._encoder_stack(sd, rows[b:b + 1, :n], 4, 4, O.Cfg(training=False)) for b, n in enumerate(N_SHORT)]


@functools.lru_cache(maxsize=None)
def short_decoder_oracle():
    """The CPU oracle's decoder output of every clip alone, on its own rows of the content embeddings."""
    _, cls, rows = short_inputs()
    sd = OL.seeded_model_state("decoder", requires_grad=False)
    with torch.no_grad():
        return [O.decoder_forward(sd, rows[b:b + 1, :n], cls[b:b + 1], O.Cfg(training=False), target_length=n)
                for b, n in enumerate(N_SHORT)]


def test_seeds_show_a_missing_mask():
    """The device tests assert that the padded batch WITHOUT lengths misses the 1e-3 bound on a shorter clip.  Here the oracle
    says that these inputs make it so with room to spare, at least 10 x the bound on every shorter clip (measured: transformer
    stack 0.89 / 0.33, decoder 0.35 / 0.20), while the full-length clip does not depend on its neighbours."""
    _, cls, rows = short_inputs()
    cfg = O.Cfg(training=False)
    with torch.no_grad():
        tp = O._encoder_stack(OL.seeded_model_state("content", requires_grad=False), rows, 4, 4, cfg)
        dp = O.decoder_forward(OL.seeded_model_state("decoder", requires_grad=False), rows, cls, cfg, target_length=3)
    for name, padded, solo in (("transformer stack", tp, short_transformer_oracle()), ("decoder", dp, short_decoder_oracle())):
        gaps = [_rel(padded[b:b + 1, :n], solo[b]) for b, n in enumerate(N_SHORT)]
        print(name, "padded batch without lengths against each clip alone:", gaps)
        assert gaps[0] < 1e-5 and min(gaps[1:]) > 1e-2, (name, gaps)
