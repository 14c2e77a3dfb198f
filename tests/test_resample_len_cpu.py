"""Native-rate, stereo recordings without a GPU: the host argument checks of ast_resample_poly_len (every bad call is refused
before any launch), the output-count formula, pad_waveforms with channels, and transfer's argument errors.  The shapes and the
float64 restatement that tests/test_gpu_resample_len.py compares the kernels against live here as well."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from ast_amd import _lib
from ast_amd import cqt
from ast_amd import utilityFunctions as U
from ast_amd.infer import StyleTransferSession

FAKE = 0x10000                                            # an aligned non-null pointer; nothing dereferences it
NEW = 22050
# rate -> (orig, new) against 22 050 Hz: the staged polyphase kernel (down and up), the 2:1 path, the unstaged kernel (klen > 638)
RATES = {48000: (320, 147), 44100: (2, 1), 16000: (320, 441), 96000: (640, 147)}


def ratio(rate):
    g = math.gcd(rate, NEW)
    return rate // g, NEW // g


def m_of(n, rate):
    orig, new = ratio(rate)
    return int(math.ceil(Fraction(n * new, orig)))


def test_ratios_and_banks():
    for rate, (orig, new) in RATES.items():
        assert ratio(rate) == (orig, new)
    shapes = {rate: (cqt._sinc_bank(*ratio(rate))[0].shape, cqt._sinc_bank(*ratio(rate))[1]) for rate in RATES}
    assert shapes == {48000: ((147, 348), 14), 44100: ((1, 28), 13), 16000: ((441, 334), 7), 96000: ((147, 694), 27)}


def test_output_count_closed_form():
    """m_b = (n_b * new + orig - 1) // orig, the integer form the kernels use, against math.ceil of the exact quotient and
    against what `resample` allocates, for every n_b in 1 .. 2000 and at the 2^31 end of the accepted range."""
    for rate in (48000, 44100, 16000):
        orig, new = ratio(rate)
        for nb in range(1, 2001):
            want = math.ceil(Fraction(nb * new, orig))
            assert (nb * new + orig - 1) // orig == want == cqt.resampled_length(nb, rate, NEW), (rate, nb)
            assert int(math.ceil(new * nb / orig)) == want                      # cqt.resample's own count
        nb = (2 ** 31 - 1) // new
        assert cqt.resampled_length(nb, rate, NEW) == math.ceil(Fraction(nb * new, orig))
    assert cqt.resampled_length(85760, NEW, NEW) == 85760


def _call(lib, **kw):
    a = dict(x=FAKE, B=4, C=2, n=6000, kern=FAKE, orig=320, new=147, klen=348, width=14, y=FAKE, m=m_of(6000, 48000), gain=1.0,
             n_in=FAKE, n_out=FAKE)
    a.update(kw)
    return lib.ast_resample_poly_len(a["x"], a["B"], a["C"], a["n"], a["kern"], a["orig"], a["new"], a["klen"], a["width"], a["y"],
                                     a["m"], a["gain"], a["n_in"], a["n_out"], None)


def test_entry_refuses_bad_arguments():
    lib = _lib.lib()
    big = (2 ** 31 - 1) // 147 + 1                                               # n * new reaches 2^31
    for kw, needle in ((dict(x=None), b"null"), (dict(kern=None), b"null"), (dict(y=None), b"null"), (dict(B=0), b"bad shape"),
                       (dict(B=65536), b"bad shape"), (dict(n=0), b"bad shape"), (dict(orig=0), b"bad shape"), (dict(new=0), b"bad shape"),
                       (dict(klen=0), b"bad shape"), (dict(width=-1), b"bad shape"), (dict(m=0), b"bad shape"),
                       (dict(C=0), b"channels"), (dict(C=3), b"channels"),
                       (dict(m=m_of(6000, 48000) - 1), b"ceil"), (dict(m=m_of(6000, 48000) + 1), b"ceil"),
                       (dict(n=big, m=m_of(big, 48000)), b"too long"),
                       (dict(n=2 ** 30, C=2, orig=2, new=1, klen=30, m=2 ** 29), b"too long"),                  # C * n
                       (dict(n=2 ** 31 - 400, C=1, orig=2, new=1, klen=4097, m=2 ** 30 - 200), b"too long")):   # n + 66 orig + klen
        rc = _call(lib, **kw)
        assert rc != 0, kw
        err = lib.ast_last_error()
        assert b"ast_resample_poly_len" in err and needle in err, (kw, err)


def test_valid_calls_pass_the_checks_up_to_the_launch():
    """Valid calls of the three routes (staged, 2:1, unstaged) with and without the optional pointers: without a device the
    failure is the runtime's, with one they run on zeroed buffers."""
    lib = _lib.lib()
    gpu = torch.cuda.is_available()
    routes = ((320, 147, 348, 14, 48000), (2, 1, 28, 13, 44100), (640, 147, 694, 27, 96000))
    for orig, new, klen, width, rate in routes:
        for C, lens in ((1, True), (2, True), (2, False)):
            if gpu:
                x, kern = torch.zeros(4 * C * 6000, device="cuda"), torch.zeros(new * klen, device="cuda")
                y, cnt = torch.zeros(4 * m_of(6000, rate), device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda")
                ptrs = dict(x=x.data_ptr(), kern=kern.data_ptr(), y=y.data_ptr(), n_in=cnt.data_ptr(), n_out=cnt.data_ptr() + 16)
            else:
                ptrs = {}
            if not lens:
                ptrs.update(n_in=None, n_out=None)
            rc = _call(lib, C=C, orig=orig, new=new, klen=klen, width=width, m=m_of(6000, rate), **ptrs)
            if gpu:
                assert rc == 0, (rate, C, lens, lib.ast_last_error())
                continue
            assert rc != 0
            err = lib.ast_last_error()
            for word in (b"bad", b"null", b"too long", b"ceil", b"channels"):
                assert word not in err, (rate, C, lens, err)
    if gpu:
        torch.cuda.synchronize()


def test_pad_waveforms_with_channels():
    gen = torch.Generator().manual_seed(5)
    for C in (1, 2):
        clips = [torch.randn(C, 5, generator=gen), torch.randn(C, 9, generator=gen), torch.randn(C, 1, generator=gen)]
        waves, n = U.pad_waveforms(clips, channels=C)
        assert waves.shape == (3, C, 9) and waves.dtype == torch.float32 and n.dtype == torch.int32 and n.tolist() == [5, 9, 1]
        for b, c in enumerate(clips):
            assert torch.equal(waves[b, :, :n[b]], c) and float(waves[b, :, n[b]:].abs().sum()) == 0.0
    # without `channels`: exactly what it returned before
    flat = [torch.randn(5, generator=gen), torch.randn(1, 9, generator=gen)]
    waves, n = U.pad_waveforms(flat)
    assert waves.shape == (2, 9) and n.tolist() == [5, 9] and torch.equal(waves[0, :5], flat[0]) and torch.equal(waves[1], flat[1][0])
    for bad, C in (([], 2), ([torch.zeros(2, 9), torch.zeros(1, 9)], 2), ([torch.zeros(9)], 1), ([torch.zeros(3, 9)], 3),
                   ([torch.zeros(2, 0)], 2), ([torch.zeros(2, 9, dtype=torch.float64)], 2), ([np.zeros((2, 9), dtype=np.float32)], 2)):
        with pytest.raises(ValueError):
            U.pad_waveforms(bad, channels=C)
    with pytest.raises(ValueError):
        U.pad_waveforms([torch.zeros(2, 9)])


def test_transfer_argument_errors():
    """The host refuses more than two channels and rows whose resampled length is below the front end's NS_MIN (36 608), before
    it looks for a device."""
    sess = StyleTransferSession(torch.nn.Identity(), torch.nn.Identity(), use_graph=False)
    cls = torch.zeros(2, 256)
    with pytest.raises(ValueError, match="one or two channels"):
        sess.transfer(torch.zeros(2, 3, 90000), cls, sample_rate=48000)
    assert m_of(79689, 48000) == 36608 and m_of(79688, 48000) == 36607
    with pytest.raises(ValueError, match="36608"):
        sess.transfer(torch.zeros(2, 2, 79688), cls, sample_rate=48000)
    with pytest.raises(ValueError, match="36608"):
        sess.transfer(torch.zeros(2, 1, 36607), cls)                             # (B, C, n) at 22 050 Hz takes the same route
    with pytest.raises(ValueError, match="sample_rate"):
        sess.transfer(torch.zeros(2, 2, 90000), cls, sample_rate=0)
    with pytest.raises(ValueError, match="float32"):
        sess.transfer(torch.zeros(2, 2, 2, 90000), cls, sample_rate=48000)
    with pytest.raises(ValueError, match="cuda"):
        sess.transfer(torch.zeros(2, 2, 79689), cls, sample_rate=48000)          # long enough: only the device is missing
    for bad in ((torch.zeros(2, 3, 600),), (torch.zeros(600),), (torch.zeros(2, 600, dtype=torch.float64),)):
        with pytest.raises(ValueError):
            cqt.resample_batch(*bad, None, 48000)


# ---- shared with tests/test_gpu_resample_len.py ------------------------------------------------------------------------------------
def polyphase_f64(x, rate):
    """float64 restatement of the polyphase sum on one mono clip: y[i * new + p] = sum_k kern[p][k] x[i * orig + k - width], x = 0
    outside the clip, with the float32 bank the device uses (the bank's own rounding is not the kernel's error)"""
    orig, new = ratio(rate)
    kern, width = cqt._sinc_bank(orig, new)
    x = np.asarray(x, dtype=np.float64)
    m = m_of(len(x), rate)
    rows = -(-m // new)
    xp = np.concatenate([np.zeros(width), x, np.zeros(rows * orig + kern.shape[1])])
    frames = np.lib.stride_tricks.sliding_window_view(xp, kern.shape[1])[::orig][:rows]       # (rows, klen)
    return (frames @ kern.astype(np.float64).T).reshape(-1)[:m]
