"""ast_resample_poly_len / cqt.resample_batch on the device: load_audio's resample and stereo mean for a padded batch of clips at
their native rate, and StyleTransferSession.transfer(..., sample_rate=) with that step inside the captured graph.

Operator shape: B = 6 rows of n = 45 003 samples holding 6000, 1, 13, 3333, 20 480 and 45 003.  Tiles (csrc/cqt.hip): the staged
kernel (48 kHz: 320 -> 147, 16 kHz: 320 -> 441) gives a workgroup 64 / C polyphase rows = (64 / C) * new outputs = (64 / C) * 320
input samples; the 2:1 path (44.1 kHz) 256 outputs at this size (1024 from B * m = 256 Ki outputs on: its own test); the unstaged
kernel (96 kHz: 694 taps, more than a row of LDS per lane) has none.  20 480 = 64 * 320 = 40 * 512 samples end on a tile boundary
of all of them, 45 003 span three tiles or more; both are asserted.

Bounds.  Against `cqt.resample` (and torch.mean over the channels) on each clip alone: bit equality, the same sums in the same
order.  Against the float64 restatement of the polyphase sum (test_resample_len_cpu.polyphase_f64): 3 x the error `cqt.resample`
itself shows against it on these clips, the margin being for the mean's one extra rounding."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import ast_amd
    from ast_amd import config, cqt
    from ast_amd import utilityFunctions as U
    from ast_amd.infer import StyleTransferSession
from oracle import seeded_params as sp
from test_resample_len_cpu import NEW, m_of, polyphase_f64, ratio

DEV = "cuda"
N = 45003
N_IN = [6000, 1, 13, 3333, 20480, 45003]
RATES = (48000, 44100, 16000, 96000)
BOUND_SESSION_F32 = 5.3e-6                     # tests/test_gpu_ragged_wave.py: 10 x the f32 session's composition noise


def i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def rel_err(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / max(b.abs().max().item(), 1e-12))


def tile_outputs(rate, C, B, m):
    """outputs one workgroup owns (None: the unstaged kernel)"""
    orig, new = ratio(rate)
    if (orig, new) == (2, 1):
        return 1024 if B * m >= 256 * 1024 else 256
    klen = cqt._sinc_bank(orig, new)[0].shape[1]
    return None if klen > 638 else (64 // C) * new


def batch(C, seed=0, fill=0.0, n_in=N_IN, n=N):
    """(B, C, n) seeded clips, `fill` behind every clip's end"""
    gen = torch.Generator().manual_seed(100 + seed)
    x = torch.randn(len(n_in), C, n, generator=gen)
    for b, nb in enumerate(n_in):
        x[b, :, nb:] = fill
    return x.to(DEV)


def solo(x, n_in, rate):
    """every clip alone through the existing path: cqt.resample on its (C, n_b) samples, then load_audio's mean"""
    return [torch.mean(cqt.resample(x[b, :, :nb].contiguous(), rate, NEW), dim=0) for b, nb in enumerate(n_in)]


def run(x, n_in, rate):
    y, n_out = cqt.resample_batch(x if x.shape[1] == 2 else x[:, 0].contiguous(), n_in, rate, NEW)
    return y.clone(), (None if n_out is None else n_out.clone())


@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("rate", RATES)
def test_rows_are_each_clip_alone(rate, C):
    x = batch(C)
    B, m = len(N_IN), m_of(N, rate)
    want_n = [m_of(nb, rate) for nb in N_IN]
    tile = tile_outputs(rate, C, B, m)
    if tile is not None:
        assert want_n[4] % tile == 0 and -(-want_n[5] // tile) >= 3, (tile, want_n)
    y, n_out = run(x, i32(N_IN), rate)
    assert y.shape == (B, m) and n_out.dtype == torch.int32 and n_out.tolist() == want_n
    ref = solo(x, N_IN, rate)
    for b, mb in enumerate(want_n):
        assert ref[b].shape == (mb,)
        assert torch.equal(y[b, :mb], ref[b]), f"clip {b} (n_b = {N_IN[b]}): {float((y[b, :mb] - ref[b]).abs().max())}"
        if mb < m:
            assert float(y[b, mb:].abs().max()) == 0.0, f"tail of clip {b}"
    # whatever lies behind a clip's end is never read
    yn, nn = run(batch(C, fill=float("nan")), i32(N_IN), rate)
    assert torch.equal(yn, y) and torch.equal(nn, n_out)
    # two runs are bitwise equal
    y2, _ = run(x, i32(N_IN), rate)
    assert torch.equal(y2, y)
    # out-of-range device values equal the clamped ones
    yc, nc = run(x, i32([0, -5, N + 9, 3333, 20480, 2 ** 31 - 1]), rate)
    yw, nw = run(x, i32([1, 1, N, 3333, 20480, N]), rate)
    assert torch.equal(yc, yw) and nc.tolist() == nw.tolist() == [m_of(v, rate) for v in (1, 1, N, 3333, 20480, N)]
    # without lengths every clip is n long, and so says n_out
    full = batch(C, seed=1, n_in=[N] * B)
    ya, na = run(full, None, rate)
    yb, nb_ = run(full, i32([N] * B), rate)
    assert torch.equal(ya, yb) and na.tolist() == nb_.tolist() == [m] * B
    if C == 1:                                                           # a full batch is the plain entry's, row for row
        assert torch.equal(ya, cqt.resample(full[:, 0].contiguous(), rate, NEW))
    # the same through the C-ABI without n_out
    from ast_amd._lib import check, lib, ptr, stream
    orig, new = ratio(rate)
    kern, width = cqt._device_sinc_bank(orig, new, str(x.device))
    y3 = torch.full((B, m), float("nan"), device=DEV)
    xin = (x if C == 2 else x[:, 0]).contiguous()
    check(lib().ast_resample_poly_len(ptr(xin), B, C, N, ptr(kern), orig, new, kern.shape[1], width, ptr(y3), m, 1.0, ptr(i32(N_IN)), None,
                                      stream()), "ast_resample_poly_len")
    assert torch.equal(y3, y)


@pytest.mark.parametrize("rate", RATES)
def test_against_the_float64_polyphase_sum(rate):
    """valid samples against the float64 restatement; the bound is 3 x the existing resampler's own error on these clips"""
    x = batch(2)
    y2, _ = run(x, i32(N_IN), rate)
    y1, _ = run(x[:, :1].contiguous(), i32(N_IN), rate)
    e_old = e_mono = e_stereo = 0.0
    for b, nb in enumerate(N_IN):
        f64 = [polyphase_f64(x[b, c, :nb].cpu().numpy(), rate) for c in (0, 1)]
        old = cqt.resample(x[b, :, :nb].contiguous(), rate, NEW).double().cpu().numpy()
        e_old = max(e_old, float(np.abs(old - np.stack(f64)).max()))
        mb = m_of(nb, rate)
        e_mono = max(e_mono, float(np.abs(y1[b, :mb].double().cpu().numpy() - f64[0]).max()))
        e_stereo = max(e_stereo, float(np.abs(y2[b, :mb].double().cpu().numpy() - 0.5 * (f64[0] + f64[1])).max()))
    print(f"{rate} Hz against the float64 polyphase sum: cqt.resample {e_old:.3g}, resample_batch mono {e_mono:.3g}, stereo {e_stereo:.3g} "
          f"(bound {3 * e_old:.3g})")
    assert e_old > 0.0 and e_mono <= 3 * e_old and e_stereo <= 3 * e_old


def test_halving_with_four_outputs_per_thread():
    """44.1 kHz from B * m = 256 Ki outputs on: the 2:1 path's other instantiation (1024 outputs per workgroup)"""
    n, n_in = 131072, [131072, 100001, 2048, 1]
    x = batch(2, seed=2, fill=float("nan"), n_in=n_in, n=n)
    assert tile_outputs(44100, 2, 4, m_of(n, 44100)) == 1024 and m_of(2048, 44100) == 1024
    y, n_out = run(x, i32(n_in), 44100)
    assert n_out.tolist() == [m_of(v, 44100) for v in n_in]
    for b, ref in enumerate(solo(x, n_in, 44100)):
        assert torch.equal(y[b, :ref.shape[0]], ref), b
        assert ref.shape[0] == y.shape[1] or float(y[b, ref.shape[0]:].abs().max()) == 0.0


def test_equal_rates():
    x = batch(2, seed=3, fill=float("nan"))
    mono = x[:, 0].contiguous()
    n = i32(N_IN)
    y, n_out = cqt.resample_batch(mono, n, NEW, NEW)
    assert y is mono and n_out is n
    y, n_out = cqt.resample_batch(x, n, NEW, NEW)
    assert n_out.tolist() == N_IN
    for b, nb in enumerate(N_IN):
        assert torch.equal(y[b, :nb], torch.mean(x[b, :, :nb], dim=0)) and (nb == N or float(y[b, nb:].abs().max()) == 0.0)


# ---- session -----------------------------------------------------------------------------------------------------------------------
def _seeded(tag, ctor):
    m = ctor()
    m.load_state_dict(sp.seeded_state_dict(m.state_dict(), tag=tag))
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
        if isinstance(mod, torch.nn.MultiheadAttention):
            mod.dropout = 0.0
    return m.to(DEV).eval()


def _longest(target, rate):
    """the largest sample count at `rate` that resamples to `target` samples"""
    orig, new = ratio(rate)
    n = target * orig // new
    assert m_of(n, rate) == target and m_of(n + 1, rate) == target + 1
    return n


def _transfer_check(bound):
    rate, targets = 48000, (85760, 36708)                             # the existing tests' 2-section clip and a short one
    n_in = [_longest(t, rate) for t in targets]
    gen = torch.Generator().manual_seed(77)
    clips = [(0.1 * torch.randn(2, nb, generator=gen)).to(DEV) for nb in n_in]
    enc, dec = _seeded("content", ast_amd.ContentEncoder), _seeded("decoder", ast_amd.Decoder)
    cls = sp.seeded_normal((2, 256), 7710).to(DEV)
    old = StyleTransferSession(enc, dec, use_graph=False)
    eager, graph = StyleTransferSession(enc, dec, use_graph=False), StyleTransferSession(enc, dec, use_graph=True)
    seen = 0.0
    for k, order in enumerate(([0, 1], [1, 0])):                      # the second call: clips swapped, NaN behind their ends
        mono = [torch.mean(cqt.resample(clips[b], rate, NEW), dim=0) for b in order]
        assert [int(w.shape[0]) for w in mono] == [targets[b] for b in order]
        w_ref, n_ref = U.pad_waveforms(mono)
        ref = tuple(t.clone() for t in old.transfer(w_ref, cls, n_samples=n_ref))
        waves, n = U.pad_waveforms([clips[b] for b in order], channels=2)
        assert waves.shape == (2, 2, max(n_in)) and n.tolist() == [n_in[b] for b in order]
        if k:
            for row, b in enumerate(order):
                waves[row, :, n_in[b]:] = float("nan")
        y, n_out = cqt.resample_batch(waves, n, rate, NEW)
        assert torch.equal(y, w_ref) and torch.equal(n_out, n_ref)
        for sess in (eager, graph):
            res = tuple(t.clone() for t in sess.transfer(waves, cls, n_samples=n, sample_rate=rate))
            assert len(res) == 3 and res[0].shape == ref[0].shape and res[1].shape == ref[1].shape
            assert torch.equal(res[2], ref[2]) and bool(torch.isfinite(res[0]).all())
            for row in range(2):
                L = int(ref[2][row])
                e = max(rel_err(res[0][row, :L], ref[0][row, :L]), rel_err(res[1][row], ref[1][row]))
                seen = max(seen, e)
                assert e <= bound, (order, row, e)
                assert L == res[0].shape[1] or float(res[0][row, L:].abs().max()) == 0.0
        assert len(graph._graphs) == 1                                # both mixes replay the one graph
    print(f"transfer from 48 kHz stereo ({config.compute_dtype}): largest deviation from resample -> mean -> transfer {seen:.3g} (bound {bound:.1e})")
    return graph, waves, cls, n


def test_transfer_native_rate_f32():
    config.set_compute_dtype(torch.float32)
    graph, waves, cls, n = _transfer_check(BOUND_SESSION_F32)
    # (B, n) rows at 22 050 Hz keep their key and path: a second graph, keyed as before this argument existed
    mono = torch.zeros(2, 85760, device=DEV)
    graph.transfer(mono, cls)
    keys = sorted(graph._graphs, key=len)
    assert len(keys) == 2 and keys[1][-2:] == (48000, 2) and keys[1][:-2][1:] == keys[0][1:] and keys[0][0] == (2, 85760)


def test_transfer_native_rate_bf16():
    config.set_compute_dtype(torch.bfloat16)
    try:
        _transfer_check(0.0)
    finally:
        config.set_compute_dtype(torch.float32)
