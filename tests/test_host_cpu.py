"""CPU-only checks of the host side: the C-ABI library loads and exports every symbol the
header declares, module state_dict layouts equal the reference's, geometry builders are
consistent, and the product path refuses to run without a GPU (no fallback)."""
import os
import re

import pytest
import torch

import ast_amd
from ast_amd import _lib, ops
from oracle import layout as OL
from oracle import seeded_params as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "ast_hip.h")).read()
    declared = set(re.findall(r"\b(ast_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.EXPORTS), (declared ^ set(_lib.EXPORTS))
    lib = _lib.lib()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.ast_version() >= 100


def test_state_dict_layouts_match_reference(golden_dir):
    import numpy as np
    g = np.load(os.path.join(golden_dir, "model_b2s2.npz"))
    for tag, ctor in (("style", ast_amd.StyleEncoder), ("content", ast_amd.ContentEncoder),
                      ("decoder", ast_amd.Decoder), ("disc", ast_amd.Discriminator)):
        m = ctor()
        assert sp.layout_digest(m.state_dict()) == str(g[f"digest_{tag}"]) == sp.layout_digest(OL.LAYOUTS[tag]())
    # fresh decoder: every 1-D `*weight*` zero (new_decoder.py:134-143)
    dec = ast_amd.Decoder()
    assert all(float(p.abs().max()) == 0.0 for n, p in dec.named_parameters() if p.dim() == 1 and "weight" in n)
    assert float(dec.start_token.abs().max()) > 0.0
    # positional table is the reference's closed form
    pe = ast_amd.SinusoidalPositionalEncoding(256).pe
    assert torch.allclose(pe, OL.style_encoder_layout()["pos_encoder.pe"], atol=1e-6)


def test_no_cpu_fallback():
    with pytest.raises(RuntimeError, match="device tensors"):
        ast_amd.StyleEncoder()(torch.randn(1, 1, 2, 287, 597))
    with pytest.raises(RuntimeError, match="device tensors"):
        ast_amd.compute_comprehensive_loss(torch.randn(1, 1, 2, 8, 8), torch.randn(1, 1, 2, 8, 8))


def _taps(g):
    return [((g.tap[i] & 255) - 64, ((g.tap[i] >> 8) & 255) - 64, g.tap[i] >> 16) for i in range(g.ntaps)]


@pytest.mark.parametrize("H,W,k,s,p", [(287, 597, 3, 2, 1), (144, 299, 3, 1, 1), (9, 19, 1, 2, 0), (5, 10, 3, 2, 1), (36, 65, 3, 2, 1)])
def test_gather_geometry_covers_every_tap_once(H, W, k, s, p):
    """The transposed (data-gradient / ConvTranspose) launches together must enumerate exactly the
    (input pixel, output pixel, tap) triples of the direct convolution."""
    gd, (Ho, Wo) = ops.gather_direct(1, H, W, 8, 8, k, s, p)
    direct = set()
    for ho in range(Ho):
        for kh in range(k):
            hi = ho * s - p + kh
            if 0 <= hi < H:
                direct.add((hi, ho, kh))
    trans = set()
    for g in ops.gathers_transposed(1, Ho, Wo, 8, H, W, 8, k, s, p):
        for hm in range(g.Hm):
            hd = hm * g.dsh + g.doh
            assert 0 <= hd < H
            for dh, dw, wt in _taps(g):
                hs = hm * g.sh + g.oh + dh
                if 0 <= hs < Ho and dw == _taps(g)[0][1]:
                    trans.add((hd, hs, wt // k))
    assert trans == direct


def test_section_bookkeeping():
    from ast_amd import utilityFunctions as U
    from oracle import frontend_oracle as FO
    for secs in (2, 3, 4, 5, 6, 7, 8, 10):
        T = 1 + (secs * 22050) // 256
        assert U.section_starts(T) == FO.section_starts(T)
    with pytest.raises(ValueError):
        U.concat_stft_cqt(torch.zeros(2, 5, 3), torch.zeros(2, 6, 3))


def test_cqt_oracle_known_answers_and_reference_shape():
    """get_CQT (utilityFunctions.py:39-60) has no golden vector (librosa absent, parity unpinned); what can be pinned
    is librosa's documented behaviour: a unit cosine at bin k's centre frequency peaks in bin k with magnitude
    sqrt(length_k)/2 (scale=True, norm=1), and the reference's own test pins the shape (2, 862, 84) for 10 s."""
    import numpy as np
    from oracle import cqt_oracle as CO
    sr = 22050
    freqs = 32.70319566257483 * 2.0 ** (np.arange(84) / 12)
    lengths, cutoff = CO.wavelet_lengths(freqs, sr, 12)
    assert cutoff < sr / 2
    t = np.arange(2 * sr) / sr
    for k in (7, 43, 81):
        mag = np.abs(CO.cqt(np.cos(2 * np.pi * freqs[k] * t)))[:, 86]
        assert mag.argmax() == k
        assert abs(mag[k] / (np.sqrt(lengths[k]) / 2) - 1) < 2e-3
    out = CO.get_cqt(np.zeros((1, 10 * sr), dtype=np.float32))
    assert out.shape == (2, 862, 84) and out.dtype == np.float32        # test_correctness.ipynb cell 3
    assert CO.get_cqt(np.zeros(4 * sr, dtype=np.float32)).shape == (2, 345, 84)
    # the stand-in decimator: unit DC gain, > 110 dB down from the new Nyquist on
    h = CO.halfband()
    H = np.abs(np.fft.rfft(h, 1 << 15))
    f = np.arange(len(H)) / (1 << 15)
    assert abs(h.sum() - 1) < 1e-12 and H[f >= 0.25].max() < 10 ** (-110 / 20) and abs(H[f <= 0.913 * 0.25] - 1).max() < 1e-4


def test_cqt_plan_folds_librosa_steps_exactly():
    """The product's per-octave correlation kernels (ast_amd/cqt.py: sparsified wavelet FFT folded with the rectangular
    STFT) reproduce the oracle's step-by-step librosa pipeline to rounding, and its resampler bank reproduces
    torchaudio's kernel formula as the oracle applies it."""
    import numpy as np
    from ast_amd import cqt as C
    from oracle import cqt_oracle as CO
    from oracle import frontend_oracle as FO
    p = C._plan(22050.0, 84, 256)
    assert p["nfft"] == 256 and [(lo, nb, h) for lo, nb, _, h, _ in p["octaves"]] == [(72 - 12 * o, 12, 256 >> o) for o in range(7)]
    y = FO.synth_waveform(1, "violin", seconds=1.0).reshape(-1).astype(np.float64)
    ref = CO.cqt(y)
    T, out, yy = 1 + len(y) // 256, np.zeros_like(ref), y
    taps = p["taps"]
    c = (len(taps) - 1) // 2
    for i, (lo, nb, rows, hop, sc) in enumerate(p["octaves"]):
        yp = np.pad(yy, (128, 128 + hop))
        frames = np.stack([yp[t * hop:t * hop + 256] for t in range(T)])
        out[lo:lo + nb] = (p["W"][rows] @ frames.T) * sc[:, None]
        ypad = np.pad(yy, (c, c + 2))
        yy = np.array([np.dot(taps, ypad[2 * j:2 * j + len(taps)]) for j in range((len(yy) + 1) // 2)]) * np.sqrt(2)
    assert np.abs(out - ref).max() / np.abs(ref).max() < 1e-12
    # resampler bank: 48 kHz -> 22.05 kHz is 320 -> 147
    kern, width = C._sinc_bank(320, 147)
    x = np.random.default_rng(3).standard_normal(3000)
    refr = CO.sinc_resample(x, 48000, 22050)
    xp = np.pad(x, (width, width + 320 + kern.shape[1]))
    got = np.array([np.dot(kern[j % 147].astype(np.float64), xp[(j // 147) * 320:(j // 147) * 320 + kern.shape[1]]) for j in range(len(refr))])
    assert np.abs(got - refr).max() < 1e-6 and len(refr) == int(np.ceil(147 * 3000 / 320))


def test_length_bucket_sampler_and_section_counts():
    """BASELINE configs[4]: clip lengths 2..8 s give S = 1,1,2,2,2,3,3 (utilityFunctions.py:246-262) and the
    sampler only ever mixes clips of one length in a batch."""
    from ast_amd.dataloader import LengthBucketSampler, sections_for_samples
    secs = [2, 3, 4, 5, 6, 7, 8, 10]
    assert [sections_for_samples(s * 22050) for s in secs] == [1, 1, 2, 2, 2, 3, 3, 4]
    lengths = [s * 22050 for s in (2, 4, 4, 7, 2, 4, 7, 2, 4, 2, 7, 7, 4, 3)]
    sm = LengthBucketSampler(lengths, batch_size=2, shuffle=True, seed=3)
    batches = list(sm)
    assert len(batches) == len(sm) == 2 + 2 + 2          # 4 x 2 s, 5 x 4 s (one dropped), 4 x 7 s, 1 x 3 s (dropped)
    for b in batches:
        assert len({lengths[i] for i in b}) == 1
    flat = [i for b in batches for i in b]
    assert len(set(flat)) == len(flat)
    sm.set_epoch(1)
    assert list(sm) != batches                            # reshuffled per epoch


def test_igemm_argument_validation_returns_error_codes():
    """ast_igemm / ast_igemm_bn must refuse bad workspace / statistics arguments with an error code on EVERY kernel path
    (gathered, direct, patch): a null or short workspace reaching a launch is a write through a bad device pointer, i.e. a GPU
    fault.  All of these return before any launch, so fake non-null pointers are never dereferenced (host logic only)."""
    import ctypes
    lib = _lib.lib()
    fake = 0x10000                                     # non-null, never dereferenced: every call below must fail validation
    bf16 = _lib.BF16

    def igemm(g, flags, ws, ws_floats):
        return lib.ast_igemm(fake, fake, None, fake, g, bf16, flags, ws, ws_floats, None)

    def igemm_bn(g, flags, ws, ws_floats, bn_x=fake, sc=fake, sf=fake):
        return lib.ast_igemm_bn(fake, fake, None, fake, g, bf16, flags, ws, ws_floats, bn_x, sc, sf, None)

    # (1) a split-K plan: the 3x3 conv 64 -> 8 channels on 16 x (32 x 16) pixels (spatial_projection-like, M = 8192)
    gs, _ = ops.gather_direct(16, 32, 16, 64, 8, 3, 1, 1)
    need = int(lib.ast_igemm_ws_floats(gs, bf16))
    assert need == 16 * 32 * 16 * 8, need              # the premise: this geometry splits K
    assert igemm(gs, 4, None, need) != 0               # null workspace
    assert b"workspace" in lib.ast_last_error()
    assert igemm(gs, 4, fake, need - 1) != 0           # short workspace
    assert igemm(gs, 8, fake, need) != 0               # fused forward statistics on a split plan
    assert b"split-K" in lib.ast_last_error()
    assert igemm_bn(gs, 16, fake, need) != 0           # fused backward sums on a split plan
    # (2) the gathered kernel without split: stride-2 3x3, 32 -> 64 channels on 16 x (144 x 299) (ResBlock b1 conv1)
    gg, _ = ops.gather_direct(16, 144, 299, 32, 64, 3, 2, 1)
    out = (ctypes.c_int32 * 5)()
    assert lib.ast_igemm_plan(gg, bf16, ctypes.byref(out)) == 0 and out[2] > 0 and out[3] == 1, list(out)   # gathered, no split
    assert int(lib.ast_igemm_ws_floats(gg, bf16)) == 0
    assert igemm(gg, 8, None, 64 * 64 * 2) != 0        # statistics table missing
    assert igemm(gg, 8, fake, 64 * 64 * 2 - 1) != 0    # ... too small
    assert igemm(gg, 8 | 1, fake, 64 * 64 * 2) != 0    # ... with accumulate
    assert igemm(gg, 64, fake, 16 * 64 * 2) != 0       # per-image slots without flag 8
    assert igemm(gg, 8 | 64, fake, 16 * 64 * 2 - 1) != 0
    assert igemm_bn(gg, 16, None, 64 * 64 * 3) != 0    # backward sums: table missing
    assert igemm_bn(gg, 16, fake, 64 * 64 * 3 - 1) != 0
    assert igemm_bn(gg, 16, fake, 64 * 64 * 3, bn_x=None) != 0
    assert igemm_bn(gg, 16, fake, 64 * 64 * 3, sc=None) != 0
    assert igemm_bn(gg, 16, fake, 64 * 64 * 3, sf=None) != 0
    assert igemm_bn(gg, 16 | 2, fake, 64 * 64 * 3) != 0
    # (3) the direct (LDS-free) kernel: 3x3, 8 -> 16 channels
    gd, _ = ops.gather_direct(2, 64, 64, 8, 16, 3, 1, 1)
    assert lib.ast_igemm_plan(gd, bf16, ctypes.byref(out)) == 0 and out[2] == 0, list(out)
    assert igemm(gd, 8, None, 64 * 16 * 2) != 0
    assert igemm_bn(gd, 16, fake, 64 * 16 * 3, bn_x=None) != 0
    # (4) the patch kernel keeps its own checks: stride-1 3x3, 64 -> 64 channels
    gp, _ = ops.gather_direct(16, 72, 150, 64, 64, 3, 1, 1)
    assert lib.ast_igemm_plan(gp, bf16, ctypes.byref(out)) == 0 and out[2] < 0, list(out)
    assert igemm(gp, 8, None, 64 * 64 * 2) != 0
    assert igemm(gp, 64, fake, 16 * 64 * 2) != 0       # per-image slots without flag 8: refused on the patch path as on the others
    assert igemm_bn(gp, 16, fake, 64 * 64 * 3, sf=None) != 0
    assert igemm(gp, 4096 | 8, fake, 64 * 64 * 2) != 0 and b"deterministic" in lib.ast_last_error()      # refused on the patch path too
    assert igemm(gg, 4096 | 8, fake, 64 * 64 * 2) != 0 and igemm_bn(gp, 4096 | 16, fake, 64 * 64 * 3) != 0
    # null geometry / tensors
    assert lib.ast_igemm(None, fake, None, fake, gg, bf16, 0, None, 0, None) != 0


def test_round3_entry_points_refuse_bad_arguments():
    """The entry points added in round 3 validate before they launch: null pointers, counts beyond the fixed kernel-argument
    tables, misaligned slab records.  Every call below returns an error code on the host (fake pointers are never dereferenced)."""
    import ctypes
    lib = _lib.lib()
    fake = 0x10000
    f5 = (ctypes.c_float * 5)(1, 1, 1, 1, 1)
    # ast_recon_loss_total: scratch / result / coefficient arrays are required, the target's row stride covers its bins
    rl = lambda out=fake, tgt=fake, ld=513, c=f5, i=f5, ws=fake, res=fake: lib.ast_recon_loss_total(out, tgt, ld, 2, 2, 8, 513, c, i, ws, res, None, None)
    assert rl(ws=None) != 0 and b"ast_recon_loss_total" in lib.ast_last_error()
    assert rl(res=None) != 0 and rl(out=None) != 0 and rl(c=None) != 0 and rl(i=None) != 0
    assert rl(ld=512) != 0
    # ast_set_values / ast_weighted_sum: at most AST_MAX_STEP_SCALARS (16) values / terms, all travelling as kernel arguments
    vals = (ctypes.c_float * 17)(*range(17))
    assert lib.ast_set_values(fake, vals, 17, None) != 0 and lib.ast_set_values(fake, vals, 0, None) != 0 and lib.ast_set_values(None, vals, 4, None) != 0
    terms = (ctypes.c_void_p * 17)(*([fake] * 17))
    widx = (ctypes.c_int32 * 17)(*([0] * 17))
    assert lib.ast_weighted_sum(terms, widx, 17, fake, fake, None) != 0
    widx[1] = 16
    assert lib.ast_weighted_sum(terms, widx, 2, fake, fake, None) != 0          # weight index outside the scalar table
    terms[0] = None
    widx[1] = 0
    assert lib.ast_weighted_sum(terms, widx, 2, fake, fake, None) != 0          # null term
    # ast_slab_sum: 1..48 records, 16-byte aligned bases, copies of a multiple of 4 floats
    bases = (ctypes.c_void_p * 2)(fake, fake + 4)
    sizes = (ctypes.c_int64 * 2)(64, 64)
    cnt = (ctypes.c_int32 * 2)(2, 2)
    assert lib.ast_slab_sum(bases, sizes, cnt, 0, None) != 0 and lib.ast_slab_sum(bases, sizes, cnt, 49, None) != 0
    assert lib.ast_slab_sum(bases, sizes, cnt, 2, None) != 0 and b"aligned" in lib.ast_last_error()
    sizes[0] = 6
    assert lib.ast_slab_sum(bases, sizes, cnt, 1, None) != 0
    # ast_wgrad_slab: slab count and the slices output
    g, _ = ops.gather_direct(2, 8, 8, 64, 64, 3, 1, 1)
    sl = ctypes.c_int32(0)
    assert lib.ast_wgrad_slab(fake, fake, fake, g, _lib.BF16, 0, ctypes.byref(sl), None) != 0
    assert lib.ast_wgrad_slab(fake, fake, fake, g, _lib.BF16, 4, None, None) != 0
    assert lib.ast_wgrad_slab(None, fake, fake, g, _lib.BF16, 4, ctypes.byref(sl), None) != 0      # (ast_wgrad's own null check)


# ---- the float64 gather-GEMM reference and the case table of tests/test_gpu_igemm_variants.py (tests/igemm_cases.py) ------------

def _ref_conv(N, H, W, Cs, Cd, kh, kw, stride, ph, pw, seed):
    import torch.nn.functional as F
    import igemm_cases as IC
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cs, H, W, dtype=torch.float64, generator=gen)
    w = torch.randn(Cd, Cs, kh, kw, dtype=torch.float64, generator=gen)
    b = torch.randn(Cd, dtype=torch.float64, generator=gen)
    g = IC.conv_gather(N, H, W, Cs, Cd, kh, kw, stride, ph, pw)
    y, A = IC.gather_gemm_ref(x.permute(0, 2, 3, 1), w.permute(0, 2, 3, 1).reshape(Cd, kh * kw, Cs), b, g)
    ref = F.conv2d(x, w, b, stride=stride, padding=(ph, pw)).permute(0, 2, 3, 1)
    Aref = F.conv2d(x.abs(), w.abs(), b.abs(), stride=stride, padding=(ph, pw)).permute(0, 2, 3, 1)
    return y, A, ref, Aref


@pytest.mark.parametrize("N,H,W,Cs,Cd,kh,kw,stride,ph,pw", [
    (2, 7, 9, 8, 16, 3, 3, 1, 1, 1), (2, 9, 12, 8, 8, 3, 3, 2, 1, 1), (3, 5, 6, 16, 8, 1, 1, 1, 0, 0), (2, 9, 19, 8, 8, 1, 1, 2, 0, 0),
    (2, 6, 7, 8, 24, 2, 3, 1, 1, 1), (2, 12, 11, 8, 8, 2, 3, 2, 1, 1), (1, 2, 2, 8, 8, 3, 3, 1, 1, 1)])
def test_gather_gemm_ref_matches_conv2d(N, H, W, Cs, Cd, kh, kw, stride, ph, pw):
    """gather_gemm_ref on Conv2d forward geometries (ops.gather_direct and the rectangular-kernel builder of the case table)
    against F.conv2d in float64, and its second output against the same convolution of absolute values."""
    y, A, ref, Aref = _ref_conv(N, H, W, Cs, Cd, kh, kw, stride, ph, pw, seed=11)
    assert y.shape == ref.shape
    assert float((y - ref).abs().max()) < 1e-12 and float((A - Aref).abs().max()) < 1e-12
    assert bool((A >= y.abs() - 1e-12).all())


@pytest.mark.parametrize("Hs,Ws,Hd,Wd,k,stride,pad", [(5, 7, 10, 14, 3, 2, 1), (5, 7, 9, 13, 3, 2, 1), (4, 6, 4, 6, 3, 1, 1), (4, 5, 8, 9, 1, 2, 0)])
def test_gather_gemm_ref_matches_conv_transpose2d(Hs, Ws, Hd, Wd, k, stride, pad):
    """The parity classes of ops.gathers_transposed, each written through gather_gemm_ref into one destination, assemble
    F.conv_transpose2d; pixels of the other classes are left as they were (old_dst) by every class's launch."""
    import torch.nn.functional as F
    import igemm_cases as IC
    N, Cs, Cd = 2, 8, 16
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(N, Cs, Hs, Ws, dtype=torch.float64, generator=gen)
    w = torch.randn(Cs, Cd, k, k, dtype=torch.float64, generator=gen)
    b = torch.randn(Cd, dtype=torch.float64, generator=gen)
    oph, opw = Hd - ((Hs - 1) * stride - 2 * pad + k), Wd - ((Ws - 1) * stride - 2 * pad + k)
    ref = F.conv_transpose2d(x, w, b, stride=stride, padding=pad, output_padding=(oph, opw)).permute(0, 2, 3, 1)
    wgt = w.permute(1, 2, 3, 0).reshape(Cd, k * k, Cs)
    dst = torch.full((N, Hd, Wd, Cd), 7.0, dtype=torch.float64)
    seen = torch.zeros(Hd, Wd, dtype=torch.int32)
    for g in ops.gathers_transposed(N, Hs, Ws, Cs, Hd, Wd, Cd, k, stride, pad):
        m = IC.grid_mask(g)
        new, A = IC.gather_gemm_ref(x.permute(0, 2, 3, 1), wgt, b, g)
        assert float(A[:, ~m].abs().max() if (~m).any() else 0.0) == 0.0 and float(new[:, ~m].abs().max() if (~m).any() else 0.0) == 0.0
        acc, _ = IC.gather_gemm_ref(x.permute(0, 2, 3, 1), wgt, None, g, old_dst=dst)      # accumulate form: off-grid pixels keep old_dst
        assert torch.equal(acc[:, ~m], dst[:, ~m])
        assert float((acc[:, m] - (dst[:, m] + new[:, m] - b)).abs().max()) < 1e-12
        dst[:, m] = new[:, m]
        seen += m.int()
    assert bool((seen == 1).all())
    assert float((dst - ref).abs().max()) < 1e-12
    # ReLU is applied after bias and the old value
    g = ops.gathers_transposed(N, Hs, Ws, Cs, Hd, Wd, Cd, k, stride, pad)[0]
    r, _ = IC.gather_gemm_ref(x.permute(0, 2, 3, 1), wgt, b, g, relu=True)
    p, _ = IC.gather_gemm_ref(x.permute(0, 2, 3, 1), wgt, b, g)
    assert torch.equal(r, p.clamp(min=0))


def test_igemm_case_table_plans_are_pinned():
    """Every row of the case table gets exactly the plan (ast_igemm_plan's five integers) and split-K workspace
    (ast_igemm_ws_floats) it records, under its own environment: a planner change that moves a row onto another kernel variant
    fails here, not silently in the GPU test.  Patch rows also pin the pconv_kernel instantiation (ast_pconv_variant: SLB, TM,
    TN, WALL).  Also: the table holds the configurations it is there for, every patch instantiation the planner can select by
    itself among them, bar the ones PATCH_NOT_LAUNCHED names."""
    import igemm_cases as IC
    seen, seen_pc = set(), {"f32": set(), "bf16": set()}
    for c in IC.CASES:
        with IC.case_env(c):
            plan, ws = IC.plan_of(c.gather(), c.dtype)
            pc = IC.patch_variant_of(c.gather(), c.dtype)
        assert (plan, ws) == (c.plan, c.ws), (c.name, plan, ws)
        assert pc == c.pc, (c.name, pc)
        fam = "patch" if plan[2] < 0 else ("direct" if plan[2] == 0 else "gathered")
        assert fam == c.family, c.name
        g = c.gather()
        if fam == "gathered":
            assert (ws > 0) == (plan[3] > 1), c.name
            E = 4 if c.dtype == "f32" else 8
            seen.add(("gathered", c.dtype) + plan + ((g.Cs // E) % plan[2] == 0,))
        elif fam == "direct":
            E = 4 if c.dtype == "f32" else 8
            seen.add(("direct", c.dtype, plan[0] // 64, g.Cd, (g.ntaps * (g.Cs // E) + 3) // 4))
        else:
            if plan[3] < 0:                                                           # row blocks: rows or the last fragment overhang
                assert g.Hm % -plan[0] or (-plan[0] * g.Wm) % 16, c.name
            else:                                                                     # 2-D tiles: overhang on both axes
                assert g.Hm % -plan[0] and g.Wm % 16, c.name
            assert pc and (pc[0], pc[2] * 16) == (-plan[2], plan[1]), c.name
            seen.add(("patch", c.dtype) + plan)
            seen_pc[c.dtype].add(pc)
    for dt in ("f32", "bf16"):
        for bm, bn, kch, kg, splits in ((64, 64, 4, 1, (1,)), (64, 64, 8, 1, (1,)), (64, 64, 8, 4, (1,)), (64, 128, 4, 1, (1,)), (64, 128, 8, 1, (1,)),
                                        (64, 32, 4, 1, (1, 2, 4)), (128, 32, 4, 1, (1, 2, 4)), (64, 16, 4, 1, (1, 2, 4)), (128, 16, 4, 1, (1, 2, 4))):
            for ns in splits:
                for ut in (True, False):
                    assert ("gathered", dt, bm, bn, kch, ns, kg, ut) in seen, (dt, bm, bn, kch, ns, kg, ut)
        for cd in (8, 16):
            for nks in (1, 2, 3):
                assert ("direct", dt, 1, cd, nks) in seen, (dt, cd, nks)
        for jt in (2, 4, 8):
            assert any(s[:3] == ("direct", dt, jt) for s in seen), (dt, jt)
        for plan in ((-8, 32, -64, 1, 1), (-16, 32, -64, 1, 1), (-8, 64, -64, 1, 1), (-8, 32, -128, 1, 1), (-8, 64, -128, 1, 1), (-12, 64, -128, 1, 1),
                     (-3, 32, -128, -8, 1), (-9, 32, -128, -12, 1), (-5, 32, -64, -8, 1), (-5, 32, -128, -4, 1)):
            assert ("patch", dt) + plan in seen, (dt, plan)
        assert seen_pc[dt] == IC.PATCH_SELECTABLE[dt], (dt, sorted(seen_pc[dt] ^ IC.PATCH_SELECTABLE[dt]))
    # WALL on and off on the same geometry, for each tile form WALL runs with
    for name in ("rows", "2d", "rows12", "tiny4"):
        on, off = IC.BY_NAME[f"p128-wall-{name}-bf16"], IC.BY_NAME[f"p128-nowall-{name}-bf16"]
        assert on.geom == off.geom and on.pc[3] == 1 and off.pc[3] == 0 and on.pc[:2] == off.pc[:2], name
    # what the table leaves alone is selectable (so the list is honest), and nothing else is: 64-byte slabs with WALL
    for slb_tm_tn_wall, geom in (((64, 2, 2, 1), (5, 61, 67, 160, 64, 3, 3, 1, 1, 1)), ((64, 3, 2, 1), (50, 9, 19, 160, 128, 3, 3, 1, 1, 1)),
                                 ((64, 4, 2, 1), (32, 125, 49, 160, 64, 3, 3, 1, 1, 1))):
        assert slb_tm_tn_wall in IC.PATCH_NOT_LAUNCHED["bf16"]
        probe = IC.Case("probe", "patch", "bf16", ("conv",) + geom, (), (), 0)
        with IC.case_env(probe):
            assert IC.patch_variant_of(probe.gather(), "bf16") == slb_tm_tn_wall, geom
    assert not (IC.PATCH_NOT_LAUNCHED["bf16"] & IC.PATCH_SELECTABLE["bf16"]) and len(IC.PATCH_NOT_LAUNCHED["bf16"]) == 3
    # the f32 direct rows cannot be 3x3: the library refuses 4 source channels, and 8 make 18 chunks
    import ctypes
    out = (ctypes.c_int32 * 5)()
    g4 = IC.conv_gather(2, 7, 19, 4, 8, 3, 3, 1, 1, 1)
    assert _lib.lib().ast_igemm_plan(g4, _lib.dcode(torch.float32), ctypes.byref(out)) != 0


def test_igemm_case_inputs_stay_inside_reference_assumptions():
    """What the GPU test relies on, checked for every row's seeded inputs: no reference output (plus its bound, plus an old
    value) comes near the sentinel that marks untouched memory, the bias is non-zero, and the BatchNorm pre-activation
    fma(x, scale, shift) of the backward-sums form keeps |.| > 1e-3, so that the ReLU mask cannot flip on f32 rounding."""
    import igemm_cases as IC
    for c in IC.CASES:
        g, d = c.gather(), IC.make_inputs(c)
        assert d["src"].dtype == IC.DTYPES[c.dtype] and float(d["bias"].abs().min()) >= 0.05
        assert float(IC.bn_pre(d["bn_x"], d["scale"], d["shift"]).abs().min()) > IC.MASK_MARGIN, c.name
        # A bounds |ref| for every form: products, bias and the old value, all by absolute value
        amax = (d["src"].double().abs().amax() * d["wgt"].double().abs().sum(dim=(1, 2)).amax() + d["bias"].abs().max() + d["old"].double().abs().max())
        K = g.ntaps * g.Cs
        assert float(amax) * (1 + 2 * K * IC.U24 + 2.0 ** -8) < 0.25 * abs(IC.SENTINEL), c.name
        assert float(torch.tensor(IC.SENTINEL).to(IC.DTYPES[c.dtype])) == IC.SENTINEL


def test_igemm_bound_rejects_broken_results():
    """The derived bound is not vacuous: it rejects the reference with one 16-byte K chunk dropped and with one tail pixel
    zeroed, for an f32 and a bf16 row of each kernel family; a result 0.999 of the bound away passes, 1.01 on one element fails."""
    import igemm_cases as IC
    for name in ("g128x32k4s1-div", "g64x128k8s1-shift", "d-cd8-nks3", "d-cd16-nks1", "p128-tiny4", "p64-rows8"):
        for dt in ("f32", "bf16"):
            c = IC.BY_NAME[f"{name}-{dt}"]
            g, d = c.gather(), IC.make_inputs(c)
            bf = dt == "bf16"
            ref, A = IC.gather_gemm_ref(d["src"], d["wgt"], d["bias"], g)
            bound = IC.out_bound(ref, A, g, bf)
            m = IC.grid_mask(g)
            # a result just inside the bound on every element passes, just outside on one element does not
            near = ref + 0.999 * bound
            assert bool(((near - ref).abs() <= bound)[:, m].all())
            over = ref.clone()
            hd0, wd0 = g.doh, g.dow
            over[0, hd0, wd0, 0] += 1.01 * bound[0, hd0, wd0, 0]
            assert int(((over - ref).abs() > bound).sum()) == 1
            E = 4 if dt == "f32" else 8
            w2 = d["wgt"].clone()
            w2[:, g.tap[g.ntaps - 1] >> 16, g.Cs - E:] = 0                      # the last chunk of the last tap: the K tail
            broken, _ = IC.gather_gemm_ref(d["src"], w2, d["bias"], g)
            frac = float(((broken - ref).abs() > bound)[:, m].double().mean())
            assert frac > 0.5, (c.name, frac)                                    # most outputs, not a stray one
            tail = ref.clone()
            hd, wd = (g.Hm - 1) * g.dsh + g.doh, (g.Wm - 1) * g.dsw + g.dow
            tail[g.N - 1, hd, wd, :] = 0                                         # pixel M - 1
            assert int(((tail - ref).abs() > bound).sum()) == g.Cd, c.name
