"""Restatement of the last two metrics of the reference's evaluation scripts, in a dtype of the caller's choice, on tests/mfcc_ref.py:

    onset_accuracy (evaluation_reconstruction.py:54-81): librosa.onset.onset_detect(y, sr=22050) at its defaults, then the F1 score
    self_similarity_distance (evaluation_style_transfer.py:121-133): librosa.segment.recurrence_matrix(mfcc.T) at its defaults

The chain, as the issue that asked for it pins it (librosa is not available; parity with its own output is unpinned):

    dB = mfcc_ref.mel_db at hop 512, clamped from below to the clip's own maximum - 80
    e[t] = 0 for t < 3, (1 / 128) sum_m max(0, dB[m, t-2] - dB[m, t-3]) for 3 <= t < T         (lag 1, max_size 1, mean, centred)
    no onsets if e is all zero or not all finite; else x = (e - min e) / (max(e - min e) + float32 tiny) and frame n is a detection
    if x[n] == max(x[n - pre_max .. n + post_max - 1]) and x[n] >= mean(x[n - pre_avg .. n + post_avg - 1]) + 0.07, windows cut at
    the clip's ends; walking up, a detection is kept if n > last kept + wait.  pre_max = 0.03 sr // hop = 1, post_max = 1,
    pre_avg = 0.10 sr // hop = 4, post_avg = 5, wait = 1.
    onset_accuracy: both clips cut to min(n_o, n_g) samples; 1 if both onset sets are empty, 0 if one is, else 2 |O & G| / (|O| + |G|)

    c = mfcc(y, 20, 512): the matrix's points are the 20 coefficient ROWS (the reference hands over the transpose), D[i, j] = ||c_i - c_j||
    per column j the min(19, k + 2) = 12 nearest other rows, those at distance exactly 0 dropped, of the rest the k = 10 nearest kept:
    R[i, j] = 1; not symmetrised.  self_similarity_distance = mean |R_a - R_b| over the 400 cells.

float64 is what the kernels are checked against; float32 on the CPU (the "twin") gives the rounding floor of the continuous outputs
and the size the margins of the discrete ones are measured in.  The keyword arguments shift, clamp_max, keep and sym seed mistakes.

Shared by tests/test_onset_cpu.py and tests/test_gpu_onset.py: the fixture, its counts and the references (once per process)."""
import functools
import math

import numpy as np
import torch
from sklearn.metrics import f1_score
from sklearn.neighbors import NearestNeighbors

import mfcc_ref as MF

SR, N_FFT, HOP, N_MFCC = 22050, 2048, 512, 20
SHIFT = 1 + N_FFT // (2 * HOP)                            # lag 1 + the frames center=True pads on the left
PRE_MAX, POST_MAX = int(0.03 * SR // HOP), int(0.00 * SR // HOP + 1)
PRE_AVG, POST_AVG = int(0.10 * SR // HOP), int(0.10 * SR // HOP + 1)
WAIT, DELTA = int(0.03 * SR // HOP), 0.07
WIDTH = 1
K = 2 * math.ceil(math.sqrt(N_MFCC - 2 * WIDTH + 1))     # links kept per column
NN = min(N_MFCC - 1, K + 2 * WIDTH)                      # neighbours asked of sklearn
assert (SHIFT, PRE_MAX, POST_MAX, PRE_AVG, POST_AVG, WAIT, K, NN) == (3, 1, 1, 4, 5, 1, 10, 12)

B, N_ORIG, N_GEN = 4, 12000, 11000                       # the two batches have different widths
# T = 1 + n // 512 -> 21 (above one envelope tile of 8 and no multiple; two distance chunks of 16, the last ragged), 24 (whole tiles),
# 7 (below one tile), 1 or 3 (an all-zero envelope)
COUNTS = {"constant": [10300, 11800, 3500, 1], "reflect": [10300, 11800, 3500, 1025]}
N_GENERATED = {"constant": [10300, 8200, 3500, 1], "reflect": [10300, 8200, 3500, 1025]}      # row 1: cut to T = 17


def n_frames(n):
    return 1 + n // HOP


# ---- onsets ---------------------------------------------------------------------------------------------------------------------------
def clamped_db(x, pad_mode="constant", dtype=torch.float64, clamp_max=None):
    """(128, T) numpy in `dtype`.  clamp_max: the maximum to clamp by instead of the clip's own (a seeded mistake)"""
    db = MF.mel_db(x, HOP, pad_mode, dtype)
    top = db.max() if clamp_max is None else torch.as_tensor(clamp_max, dtype=dtype)
    return torch.maximum(db, top - MF.TOP_DB).numpy()


def onset_strength(x, pad_mode="constant", dtype=torch.float64, shift=SHIFT, clamp_max=None):
    """-> (T,).  shift=1: the 3-frame shift of center=True dropped, lag alone (a seeded mistake)"""
    db = clamped_db(x, pad_mode, dtype, clamp_max)
    T = db.shape[1]
    e = np.zeros(T, dtype=db.dtype)
    if T > shift:
        e[shift:] = np.maximum(0, db[:, 1:] - db[:, :-1]).mean(axis=0)[:T - shift]
    return e


def normalised(e):
    x = e - e.min()
    return x / (x.max() + e.dtype.type(np.finfo(np.float32).tiny))


def onset_detect(e, margins=None):
    """-> (T,) bool mask.  margins: a list that receives, per frame, (|x[n] - largest other value of its maximum window|,
    |x[n] - mean - delta|, whether the second condition holds)"""
    T = len(e)
    mask = np.zeros(T, dtype=bool)
    if not np.all(np.isfinite(e)) or not e.any():
        return mask
    x = normalised(e)
    last = -np.inf
    for n in range(T):
        win = x[max(0, n - PRE_MAX):min(T, n + POST_MAX)]
        avg = x[max(0, n - PRE_AVG):min(T, n + POST_AVG)].mean()
        is_max, above = x[n] == win.max(), x[n] >= avg + x.dtype.type(DELTA)
        if margins is not None:
            others = [x[k] for k in range(max(0, n - PRE_MAX), min(T, n + POST_MAX)) if k != n]
            margins.append((min(abs(float(x[n]) - float(o)) for o in others) if others else np.inf,
                            abs(float(x[n]) - float(avg) - DELTA), bool(above)))
        if is_max and above and n > last + WAIT:
            mask[n] = True
            last = n
    return mask


def f1_formula(O, G):
    """O, G: bool masks of equal length"""
    no, ng = int(O.sum()), int(G.sum())
    if no == 0 and ng == 0:
        return 1.0
    if no == 0 or ng == 0:
        return 0.0
    return 2.0 * int((O & G).sum()) / (no + ng)


def f1_reference(frames_o, frames_g, total_frames):
    """evaluation_reconstruction.py:60-78 on two index lists, total_frames as given"""
    if len(frames_o) == 0 and len(frames_g) == 0:
        return 1.0
    if len(frames_o) == 0 or len(frames_g) == 0:
        return 0.0
    y_true, y_pred = np.zeros(total_frames), np.zeros(total_frames)
    y_true[frames_o] = 1
    y_pred[frames_g] = 1
    return float(f1_score(y_true, y_pred, average="binary"))


def onset_accuracy(a, g, pad_mode="constant", dtype=torch.float64, cut=True, **kw):
    """cut=False: the clips not cut to the common length, the masks compared over the shorter one's frames (a seeded mistake)"""
    L = min(len(a), len(g))
    if cut:
        a, g = a[:L], g[:L]
    O, G = (onset_detect(onset_strength(x, pad_mode, dtype, **kw)) for x in (a, g))
    T = min(len(O), len(G))
    return f1_formula(O[:T], G[:T])


# ---- recurrence matrix ----------------------------------------------------------------------------------------------------------------
def coef_rows(x, pad_mode="constant", dtype=torch.float64):
    return MF.mfcc(x, N_MFCC, HOP, pad_mode, dtype).numpy()


def distances2(c):
    """(20, 20) squared distances between the rows, the differences themselves summed"""
    d = c[:, None, :] - c[None, :, :]
    return (d * d).sum(axis=2)


def neighbour_rule(D, keep=K, sym=False):
    """R from a (20, 20) matrix of distances (or squared distances: the order is the same), ties to the lower index.
    keep=NN: all 12 neighbours kept; sym: symmetrised as librosa's sym=True (both seeded mistakes)"""
    t = D.shape[0]
    R = np.zeros((t, t), dtype=np.int32)
    for j in range(t):
        order = sorted((i for i in range(t) if i != j), key=lambda i: (D[i, j], i))[:NN]
        for i in [i for i in order if D[i, j] != 0][:keep]:
            R[i, j] = 1
    return np.minimum(R, R.T) if sym else R


def recurrence_sklearn(c):
    """librosa.segment.recurrence_matrix(c.T)'s steps on sklearn itself: the 12-neighbour distance graph (a point is not its own
    neighbour), explicit zeros lost, the 10 nearest links of every point kept; R[i, j] = 1 iff i is kept for j"""
    t = c.shape[0]
    graph = NearestNeighbors(n_neighbors=NN, algorithm="brute").fit(c).kneighbors_graph(mode="distance").tocsr()
    graph.eliminate_zeros()
    R = np.zeros((t, t), dtype=np.int32)
    for j in range(t):
        row = graph.getrow(j)
        links = row.indices[np.argsort(row.data, kind="stable")]
        R[links[:K], j] = 1
    return R


def recurrence(x, pad_mode="constant", dtype=torch.float64, **kw):
    return neighbour_rule(distances2(coef_rows(x, pad_mode, dtype)), **kw)


def self_similarity_distance(a, b, pad_mode="constant", dtype=torch.float64, **kw):
    return float(np.abs(recurrence(a, pad_mode, dtype, **kw) - recurrence(b, pad_mode, dtype, **kw)).mean())


# ---- the fixture ----------------------------------------------------------------------------------------------------------------------
def bursts(n, starts, freqs, seed, amps=None, tau=0.03):
    """tone bursts with an instant attack and an exponential decay over 1e-3 noise, float32"""
    amps = amps or (0.5,) * len(starts)
    gen = torch.Generator().manual_seed(seed)
    x = 1e-3 * torch.randn(n, generator=gen, dtype=torch.float64)
    t = torch.arange(n, dtype=torch.float64)
    for s, f, amp in zip(starts, freqs, amps):
        on = t >= s
        x = x + on * amp * torch.exp(-(t - s).clamp(min=0) / (tau * SR)) * torch.sin(2 * np.pi * f * (t - s) / SR)
    return x.float()


@functools.lru_cache(maxsize=None)
def fixture_waves():
    """(original (B, N_ORIG), generated (B, N_GEN)) float32.
    row 0: three bursts; generated = the same clip with the second burst two frames later: F1 strictly between 0 and 1
    row 1: three quiet bursts and a loud one behind the pair's common length (uncut, the loud one's envelope peak pushes a quiet
           onset below delta) against three others 50 dB up, different counts: clamped by the batch's maximum instead
           of its own, the quiet bursts are flat
    row 2: silence against a burst
    row 3: bursts, counts 1 / 1025: T <= 3, an all-zero envelope"""
    a, g = torch.zeros(B, N_ORIG), torch.zeros(B, N_GEN)
    a[0] = bursts(N_ORIG, (2048, 5120, 8192), (440, 660, 880), 4300)
    g[0] = bursts(N_GEN, (2048, 5120 + 2 * HOP, 8192), (440, 660, 880), 4300)
    a[1] = bursts(N_ORIG, (1536, 4096, 6656, 9728), (523, 392, 784, 330), 4301, (0.008, 0.008, 0.008, 0.5))
    g[1] = 300 * bursts(N_GEN, (1536, 4608, 6656), (587, 440, 698), 4302)
    g[2] = bursts(N_GEN, (1280,), (494,), 4303)
    a[3] = bursts(N_ORIG, (0, 512), (440, 880), 4304)
    g[3] = bursts(N_GEN, (0, 300), (660, 990), 4305)
    return a, g


def clips(pad_mode):
    """[(original clip, generated clip)] per row, each at its own count"""
    a, g = fixture_waves()
    return [(a[b, :COUNTS[pad_mode][b]], g[b, :N_GENERATED[pad_mode][b]]) for b in range(B)]


SILENT = ("orig", 2)                                      # the clip whose coefficient rows 1 .. 19 differ by rounding noise alone


def ranked_clips(pad_mode):
    """[(batch, row)] of the clips whose recurrence matrix is decided with a margin (test_onset_cpu.py asserts it): every clip but
    the silent one and, under "constant", the two one-sample clips of row 3.  Silence has c_1 .. c_19 = 0 in exact arithmetic and
    rounding noise of 1e-15 |c_0| in float64 -- not the exact zeros the issue expected --, and a single sample has a nearly flat
    spectrum, so that its rows 1 .. 19 are 1e-5 of |c_0| and the float32 twin gets the distances between them wrong by half
    their size: in both, the order of the distances is the order of the rounding errors."""
    out = [(w, b) for w in ("orig", "gen") for b in range(B) if (w, b) != SILENT]
    return [(w, b) for w, b in out if not (pad_mode == "constant" and b == 3)]


def _evaluate(pad_mode, dtype):
    """per batch and row: env, mask (each clip at its own count), coef, d2, R; per row: acc, ssd"""
    out = dict(orig=[], gen=[], acc=[], ssd=[])
    for x, y in clips(pad_mode):
        for which, w in (("orig", x), ("gen", y)):
            e = onset_strength(w, pad_mode, dtype)
            c = coef_rows(w, pad_mode, dtype)
            d2 = distances2(c)
            out[which].append(dict(env=e, mask=onset_detect(e), coef=c, d2=d2, R=neighbour_rule(d2)))
        out["acc"].append(onset_accuracy(x, y, pad_mode, dtype))
        out["ssd"].append(float(np.abs(out["orig"][-1]["R"] - out["gen"][-1]["R"]).mean()))
    return out


@functools.lru_cache(maxsize=None)
def references(pad_mode):
    return _evaluate(pad_mode, torch.float64)


@functools.lru_cache(maxsize=None)
def twin(pad_mode):
    return _evaluate(pad_mode, torch.float32)


def env_error(got, ref_env):
    """largest absolute error of an envelope relative to the clip's peak; 0 for an all-zero reference that is met exactly"""
    peak = float(np.abs(ref_env).max())
    err = float(np.abs(np.asarray(got, dtype=np.float64) - ref_env).max())
    return err / peak if peak > 0 else err


def d2_error(got, ref_d2):
    """largest absolute error of the squared distances relative to the clip's largest"""
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref_d2).max()) / float(ref_d2.max())


@functools.lru_cache(maxsize=None)
def f32_floor(pad_mode):
    """The rounding floor of the continuous outputs: the float32 twin against float64, maximum over the fixture's clips"""
    ref, f32 = references(pad_mode), twin(pad_mode)
    env = max(env_error(f32[w][b]["env"], ref[w][b]["env"]) for w in ("orig", "gen") for b in range(B))
    d2 = max(d2_error(f32[w][b]["d2"], ref[w][b]["d2"]) for w in ("orig", "gen") for b in range(B))
    return dict(env=env, d2=d2)


def bounds(pad_mode):
    """the project's rule: 10 x the float32 floor"""
    return {k: 10 * v for k, v in f32_floor(pad_mode).items()}
